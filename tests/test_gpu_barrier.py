"""The interior-point barrier layer (iem_barrier_*, csrc/iem_barrier_device.h) on the MI355X.

BITWISE against tests/barrier_reference.py (the numpy restatement, no tolerance): sigma, dcon, rhs, the five directions, the updated
state, the step lengths, the four maxima of the error block, the start projection — outputs into NaN-poisoned buffers with NaN
padding behind every vector, equality-row entries of the slack-side vectors still NaN afterwards — and the parked sums: sum |y|, the
sum of the multipliers and theta carry the bits of barrier_reference.error_sums, the restatement in the DEVICE'S ORDER
(barrier_reference.device_sum) on the object's own grid of info["workgroups"] workgroups, identical over ten calls, merit's two the
bits of error's [6], [7].  ONE EXCEPTION: sum log gap.  The device's log and numpy's need not agree in the last bit, so that column
is formed in the device's order from numpy's logs and compared within (N + 2)·2⁻⁵²·Σ|term| (barrier_reference.sum_bound), as against
math.fsum before; merit's copy still carries the bits of error's.

Models: opf_7 (every bound kind, fixed variables), farmer_5 (no equality rows, lower-only inequality rows), pandemic_20x3,
quadrotor_100 (no bounds at all) and pandemic_100x7: 12 000 entries = 47 workgroups of 256, more than one ticket group of 32, so the
sums cross a seam of iem_last_arrival (the grid is min(ceil(n / 256), 4096): no cap is in the way; the test prints it).

THE BIG SHAPES (barrier_reference.big_point): quadrotor(27 000) — 1 080 000 entries on 4096 workgroups, two trips of the stride
loop, the second rows only — and quadrotor(60 000) — 2 400 000 entries, nvar = 1 320 000 > 2²⁰, three trips, the second across the
nvar seam, the third rows (asserted and printed, with the entries per trip and branch).  At both: start, terms, step, update, error
and merit bit for bit as above; and every extreme slot (the two step lengths, the four maxima) with its deciding value planted at
either side of the nvar seam, at 2²⁰ − 1, 2²⁰, the first entry of trip three and n − 1 in turn — an extreme is order-free, so only a
deciding value ON a later trip shows a kernel that drops one; there too a NaN direction and a point exactly on its relaxed bound
(alpha_p = +0.0, update moves nothing).

THE TINY DIRECTION.  "The same direction ·1e-9 gives alpha = (1, 1) exactly" cannot hold at the shared state: ds = (dy − rs)/sigs and
dz = (mu/gap − z) − (z/gap)·d have parts that do not scale with the direction (the reference gives, for d·1e-9 at the shared state,
opf_7 (2.5e-2, 1.3e-2), farmer_5 (1.4e-2, 2.2e-2), pandemic_20x3 (7.7e-3, 4.6e-3), pandemic_100x7 (5.4e-3, 6.7e-3)), and opf_7's
fixed variables have gaps of 1.7e-9.  So that case runs at the CENTRED copy of the state — z = mu/gap, y = gs on inequality rows, where
those parts are exactly zero — with the factor 1e-9·min(1, smallest gap); what it asserts is unchanged: both step lengths are exactly
1.0, the seed survives."""
import contextlib
import ctypes as C
import math
import types

import numpy as np
import pytest

import barrier_reference as bref
import kkt_diag_reference as dref
from barrier_reference import KAPPA, MU, TAU

pytestmark = pytest.mark.gpu
MODELS = ["opf_7", "farmer_5", "pandemic_20x3", "quadrotor_100", "pandemic_100x7"]
BIG = {"quadrotor_27000": 27_000, "quadrotor_60000": 60_000}
PAD = 5
DW, DC = 1e-2, 1e-6      # delta_w = 1e-2 gives the inertia (nvar, ncon, 0) on both models of the solver tests (eigenvalues, checked on the host)
NAN = float("nan")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def nan(n):
    import torch
    return torch.full((n + PAD,), NAN, dtype=torch.float64, device="cuda")


def dev(a):
    """a host vector at the head of a NaN-poisoned buffer with PAD entries behind it"""
    import torch
    buf = nan(len(a))
    buf[:len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return buf


def host(buf, n):
    assert bool(np.isnan(buf[n:].cpu().numpy()).all()), "padding touched"
    return buf[:n].cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def point(name, seed=0):
    return bref.big_point(BIG[name]) if name in BIG else bref.barrier_point(name, seed)


@contextlib.contextmanager
def layer(name, seed=0):
    """the model handle, the raw barrier object and the shared point (a big shape: on the point's own bounds)"""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    P = point(name, seed)
    gm = ExaModel(P["core"], device=0, blob=P["blob"]) if P["blob"] is not None else ExaModel(P["core"], device=0)
    b = C.c_void_p()
    bounds = [np.ascontiguousarray(P[k], dtype=np.float64) for k in ("lvar", "uvar", "lcon", "ucon")] if name in BIG else [None] * 4
    iemlib.check(gm._L.iem_barrier_create(gm._h, *[a.ctypes.data if a is not None else None for a in bounds], bref.RELAX, C.byref(b)))
    try:
        info = iemlib.BarrierInfo()
        info.struct_size = C.sizeof(iemlib.BarrierInfo)
        iemlib.check(gm._L.iem_barrier_info(b, C.byref(info)))
        cn = P["B"]["counts"]
        S = types.SimpleNamespace(gm=gm, L=gm._L, b=b, P=P, B=P["B"], nvar=cn["nvar"], ncon=cn["ncon"], n=cn["nvar"] + cn["ncon"], check=iemlib.check,
                                  info={k: int(getattr(info, k)) for k, _ in iemlib.BarrierInfo._fields_})
        S.sizes = (S.nvar, S.ncon, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
        S.dsizes = (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
        assert S.nvar == int(gm.meta.nvar) and S.ncon == int(gm.meta.ncon)
        gm._sync_stream()
        yield S
    finally:
        iemlib.check(gm._L.iem_barrier_destroy(b))
        gm.close()


def big_facts(name, S):
    """what the big shapes are there for, asserted instead of trusted, and printed: the grid, the trips, the entries per trip and branch"""
    trips = bref.trips(S.nvar, S.n, S.info["workgroups"])
    print(f"{name}: n {S.n}, workgroups {S.info['workgroups']}, trips {len(trips)}, (variables, rows) per trip {trips}")
    assert {k: S.info[k] for k in S.B["counts"]} == S.B["counts"] and S.info["workgroups"] == min(-(-S.n // 256), 4096) == 4096
    if name == "quadrotor_60000":
        assert (S.nvar, S.ncon, S.n) == (1_320_000, 1_080_000, 2_400_000) and S.nvar > 2 ** 20
        assert len(trips) == 3 and trips[0][1] == 0 and trips[1][0] > 0 and trips[1][1] > 0 and trips[2][0] == 0 and trips[2][1] > 0
    else:
        assert S.n == 1_080_000 and S.nvar < 2 ** 20 < S.n and len(trips) == 2 and trips[1][0] == 0 and trips[1][1] > 0
    return trips


def terms(S, st, r, c, mu=MU):
    sigma, dcon, rhs = nan(S.nvar), nan(S.ncon), nan(S.n)
    S.check(S.L.iem_barrier_terms(S.b, *map(_p, st), _p(r), _p(c), mu, _p(sigma), _p(dcon), _p(rhs)))
    return sigma, dcon, rhs


def step(S, st, sol, mu=MU, tau=TAU):
    dirs = tuple(nan(k) for k in S.dsizes)
    alpha = nan(2)
    S.check(S.L.iem_barrier_step(S.b, *map(_p, st), _p(sol), mu, tau, *map(_p, dirs), _p(alpha)))
    return dirs, alpha


def update(S, st, sol, dirs, alpha, mu=MU, kappa=KAPPA):
    S.check(S.L.iem_barrier_update(S.b, *map(_p, st), _p(sol), *map(_p, dirs), _p(alpha), mu, kappa))


def error(S, st, r, c, mu=MU):
    out = nan(8)
    S.check(S.L.iem_barrier_error(S.b, *map(_p, st), _p(r), _p(c), mu, _p(out)))
    return out


def merit(S, x, s, c):
    out = nan(2)
    S.check(S.L.iem_barrier_merit(S.b, _p(x), _p(s), _p(c), _p(out)))
    return out


def state_host(S, st):
    return tuple(host(t, k) for t, k in zip(st, S.sizes))


def centred(B, st, mu=MU):
    """the copy of the state whose directions scale with sol: z = mu/gap, y = gs on inequality rows"""
    x, s, y, zL, zU, vL, vU = st
    with np.errstate(all="ignore"):
        cp = (x, s, y, np.where(B["hasL"], mu / (x - B["xl"]), NAN), np.where(B["hasU"], mu / (B["xu"] - x), NAN), np.where(B["gL"], mu / (s - B["rl"]), NAN),
              np.where(B["gU"], mu / (B["ru"] - s), NAN))
        q = bref._side(B, cp, mu)
        gaps = np.concatenate([q["dL"][B["hasL"]], q["dU"][B["hasU"]], q["eL"][B["gL"]], q["eU"][B["gU"]], [1.0]])
        return (x, s, np.where(B["eq"], y, q["nu"] - q["nl"])) + cp[3:], float(gaps.min())


@pytest.mark.parametrize("name", MODELS)
def test_bitwise_against_the_reference(name, built):
    with layer(name) as S:
        B, P = S.B, S.P
        print(name, "entries", S.n, "workgroups", S.info["workgroups"], {k: v for k, v in S.info.items() if k.startswith("n_") or k == "nz"})
        assert {k: S.info[k] for k in B["counts"]} == B["counts"] and S.info["workgroups"] == -(-S.n // 256)
        if name == "pandemic_100x7":
            assert S.n == 12000 and S.info["workgroups"] == 47
        st_h = P["state"]
        st = tuple(dev(a) for a in st_h)
        r, c = dev(P["r"]), dev(P["c"])
        poison = tuple(np.full(S.ncon, NAN) for _ in range(3))
        # terms
        got = terms(S, st, r, c)
        want = bref.terms(B, st_h, P["r"], P["c"])
        for g, w, k, what in zip(got, want, (S.nvar, S.ncon, S.n), ("sigma", "dcon", "rhs")):
            assert same_bits(host(g, k), w), what
        # the three directions
        d = np.random.default_rng(21).standard_normal(S.n)
        st_c, gmin = centred(B, st_h)
        for what, st_case, sol_h in (("random", st_h, d), ("tiny", st_c, d * (1e-9 * min(1.0, gmin)))):
            st_d, sol = tuple(dev(a) for a in st_case), dev(sol_h)
            dirs, alpha = step(S, st_d, sol)
            want_dirs, want_alpha = bref.step(B, st_case, sol_h, poison)
            a = host(alpha, 2)
            print(name, what, "alpha", a.tolist())
            for g, w, k, nm in zip(dirs, want_dirs, S.dsizes, ("ds", "dzL", "dzU", "dvL", "dvU")):
                assert same_bits(host(g, k), w), (what, nm)
            for g in (dirs[0], dirs[3], dirs[4]):
                assert bool(np.isnan(host(g, S.ncon)[B["eq"]]).all())
            assert same_bits(a, want_alpha), (what, a, want_alpha)
            if what == "tiny" or B["counts"]["nz"] == 0:
                assert a.tolist() == [1.0, 1.0]
            else:
                assert 0.0 < a[0] < 1.0 or 0.0 < a[1] < 1.0
            update(S, st_d, sol, dirs, alpha)
            new = bref.update(B, st_case, sol_h, want_dirs, want_alpha)
            for g, w, nm in zip(state_host(S, st_d), new, ("x", "s", "y", "zL", "zU", "vL", "vU")):
                assert same_bits(g, w), (what, nm)
            assert what == "tiny" or not same_bits(new[0], st_case[0])
        # a state with one entry exactly on its relaxed bound and a direction that leaves through it: alpha_p = +0.0, nothing moves
        if B["counts"]["nz"]:
            on = [a.copy() for a in st_h]
            dd = d.copy()
            i = int(np.nonzero(B["hasL"])[0][0])
            on[0][i], dd[i] = B["xl"][i], -abs(dd[i])
            st_d, sol = tuple(dev(a) for a in on), dev(dd)
            dirs, alpha = step(S, st_d, sol)
            a = host(alpha, 2)
            want_dirs, want_alpha = bref.step(B, tuple(on), dd, poison)
            print(name, "on a bound: alpha", a.tolist())
            assert same_bits(a, want_alpha) and same_bits(a[:1], [0.0])
            update(S, st_d, sol, dirs, alpha)
            for g, w, nm in zip(state_host(S, st_d), on, ("x", "s", "y", "zL", "zU", "vL", "vU")):
                assert same_bits(g, w), ("on a bound", nm)
        # a NaN in the direction (on an entry without any bound where there is one): alpha_p = +0.0, nothing moves
        free = np.nonzero(~(B["hasL"] | B["hasU"]))[0]
        dd = d.copy()
        dd[int(free[0]) if len(free) else 0] = NAN
        st_d, sol = tuple(dev(a) for a in st_h), dev(dd)
        dirs, alpha = step(S, st_d, sol)
        a = host(alpha, 2)
        print(name, "NaN direction: alpha", a.tolist())
        assert same_bits(a, bref.step(B, st_h, dd, poison)[1]) and same_bits(a[:1], [0.0])
        update(S, st_d, sol, dirs, alpha)
        for g, w, nm in zip(state_host(S, st_d), st_h, ("x", "s", "y", "zL", "zU", "vL", "vU")):
            assert same_bits(g, w), ("NaN direction", nm)
        # start: points inside, on and far outside the bounds
        rng = np.random.default_rng(2)
        x0 = P["om"].x0 + rng.standard_normal(S.nvar) * 10.0 ** rng.uniform(-3, 3, S.nvar)
        with np.errstate(invalid="ignore"):
            x0 = np.where(rng.random(S.nvar) < 0.2, np.where(B["hasL"], B["xl"], x0), x0)
            x0 = np.where(rng.random(S.nvar) < 0.2, np.where(B["hasU"], B["xu"], x0), x0)
        c0 = P["c"] + rng.standard_normal(S.ncon) * 10.0 ** rng.uniform(-3, 3, S.ncon)
        xs, cs = dev(x0), dev(c0)
        outs = [nan(k) for k in (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)]
        S.check(S.L.iem_barrier_start(S.b, _p(xs), _p(cs), *map(_p, outs), bref.PUSH, bref.FRAC))
        want = bref.start(B, x0, c0, poison)
        for g, w, k, nm in zip([xs] + outs, want, (S.nvar, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon), ("x", "s", "zL", "zU", "vL", "vU")):
            assert same_bits(host(g, k), w), ("start", nm)
        assert same_bits(host(cs, S.ncon), c0)
        if B["counts"]["nz"] == 0:      # the degenerate model: every output degenerates
            sg, dc_, rh = (host(g, k) for g, k in zip(got, (S.nvar, S.ncon, S.n)))
            assert same_bits(sg, np.zeros(S.nvar)) and same_bits(dc_, np.zeros(S.ncon)) and same_bits(rh, -np.concatenate([P["r"], P["c"] - B["ceq"]]))


@pytest.mark.parametrize("name", MODELS)
def test_error_block_and_merit(name, built):
    with layer(name) as S:
        B, P = S.B, S.P
        st_h = P["state"]
        st = tuple(dev(a) for a in st_h)
        r, c = dev(P["r"]), dev(P["c"])
        first = host(error(S, st, r, c), 8)
        head, *sums = bref.error(B, st_h, P["r"], P["c"])
        assert same_bits(first[:4], head), (first[:4], head)
        for _ in range(10):
            assert same_bits(host(error(S, st, r, c), 8), first)
        m = host(merit(S, st[0], st[1], c), 2)
        assert same_bits(m, first[6:8])
        for _ in range(10):
            assert same_bits(host(merit(S, st[0], st[1], c), 2), m)
        assert same_bits(host(error(S, st, r, c), 8), first)      # (merit shares the parked values and the tickets: they are as they were)
        check_sums(name, S, first, st_h, P["c"], sums[3])
        none = host(error(S, st, None, c), 8)
        assert math.isnan(none[0]) and same_bits(none[1:], first[1:])
        # a NaN in an input wins its maximum
        bad = P["c"].copy(); bad[0] = NAN
        assert math.isnan(host(error(S, st, r, dev(bad)), 8)[2])
        if B["counts"]["nz"] == 0:
            assert first[3] == 0.0 and first[5] == 0.0 and first[7] == 0.0 and first[1] == 0.0


@pytest.mark.parametrize("name", list(BIG))
def test_big_shapes_bitwise(name, built):
    """every kernel of the layer at a shape whose stride loop runs more than once (module docstring), bit for bit"""
    with layer(name) as S:
        B, P = S.B, S.P
        big_facts(name, S)
        st_h = P["state"]
        st = tuple(dev(a) for a in st_h)
        r, c = dev(P["r"]), dev(P["c"])
        poison = tuple(np.full(S.ncon, NAN) for _ in range(3))
        for g, w, k, what in zip(terms(S, st, r, c), bref.terms(B, st_h, P["r"], P["c"]), (S.nvar, S.ncon, S.n), ("sigma", "dcon", "rhs")):
            assert same_bits(host(g, k), w), what
        sol_h = np.random.default_rng(21).standard_normal(S.n)
        sol = dev(sol_h)
        dirs, alpha = step(S, st, sol)
        want_dirs, want_alpha = bref.step(B, st_h, sol_h, poison)
        a = host(alpha, 2)
        print(name, "alpha", a.tolist())
        for g, w, k, nm in zip(dirs, want_dirs, S.dsizes, ("ds", "dzL", "dzU", "dvL", "dvU")):
            assert same_bits(host(g, k), w), nm
        for g in (dirs[0], dirs[3], dirs[4]):
            assert bool(np.isnan(host(g, S.ncon)[B["eq"]]).all())
        assert same_bits(a, want_alpha) and 0.0 < a[0] < 1.0 and 0.0 < a[1] < 1.0, (a, want_alpha)
        # error and merit at the state, before it moves
        first = host(error(S, st, r, c), 8)
        head, *sums = bref.error(B, st_h, P["r"], P["c"])
        assert same_bits(first[:4], head), (first[:4], head)
        check_sums(name, S, first, st_h, P["c"], sums[3])
        assert same_bits(host(error(S, st, r, c), 8), first)
        assert same_bits(host(merit(S, st[0], st[1], c), 2), first[6:8])
        update(S, st, sol, dirs, alpha)
        new = bref.update(B, st_h, sol_h, want_dirs, want_alpha)
        for g, w, nm in zip(state_host(S, st), new, ("x", "s", "y", "zL", "zU", "vL", "vU")):
            assert same_bits(g, w), nm
        assert not same_bits(new[0], st_h[0]) and np.isnan(new[1][B["eq"]]).all()
        # start: points inside, on and far outside the bounds
        rng = np.random.default_rng(2)
        x0 = st_h[0] + rng.standard_normal(S.nvar) * 10.0 ** rng.uniform(-3, 3, S.nvar)
        with np.errstate(invalid="ignore"):
            x0 = np.where(rng.random(S.nvar) < 0.2, np.where(B["hasL"], B["xl"], x0), x0)
            x0 = np.where(rng.random(S.nvar) < 0.2, np.where(B["hasU"], B["xu"], x0), x0)
        c0 = P["c"] + rng.standard_normal(S.ncon) * 10.0 ** rng.uniform(-3, 3, S.ncon)
        xs, cs = dev(x0), dev(c0)
        outs = [nan(k) for k in (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)]
        S.check(S.L.iem_barrier_start(S.b, _p(xs), _p(cs), *map(_p, outs), bref.PUSH, bref.FRAC))
        for g, w, k, nm in zip([xs] + outs, bref.start(B, x0, c0, poison), (S.nvar, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon), ("x", "s", "zL", "zU", "vL", "vU")):
            assert same_bits(host(g, k), w), ("start", nm)


def planted(S, what):
    """``[(label, entry)]``: for every seam position the nearest entry that can carry `what` — "variable", "row", "inequality row",
    "bound" (an entry with a bound of its own), "lower", "upper" — asserted to be of that kind; a position whose nearest entry is
    another position's is listed once"""
    B = S.B
    no_x, no_s = np.zeros(S.nvar, dtype=bool), np.zeros(S.ncon, dtype=bool)
    mask = {"variable": np.concatenate([~no_x, no_s]), "row": np.concatenate([no_x, ~no_s]), "inequality row": np.concatenate([no_x, ~B["eq"]]),
            "bound": np.concatenate([B["hasL"] | B["hasU"], B["gL"] | B["gU"]]), "lower": np.concatenate([B["hasL"], B["gL"]]),
            "upper": np.concatenate([B["hasU"], B["gU"]])}[what]
    out, seen = [], set()
    for label, i in bref.seam_positions(S.nvar, S.n, S.info["workgroups"]).items():
        k = bref.nearest(mask, i)
        assert mask[k]
        if k not in seen:
            seen.add(k)
            out.append((f"{label} -> {k}", k))
    return out


def cut_at(S, st_h, i):
    """the one-entry cut of the bounds and of a host state at entry i, and the entry's place: (B1, st1, "x" or "s", index there)"""
    iv, ir = (np.array([i]), np.array([], dtype=np.int64)) if i < S.nvar else (np.array([], dtype=np.int64), np.array([i - S.nvar]))
    return bref.cut(S.B, iv, ir), bref.cut_state(st_h, iv, ir), iv, ir


@pytest.mark.parametrize("name", list(BIG))
def test_big_extremes_on_later_trips(name, built):
    """the two step lengths and the four maxima with their deciding value planted at each seam position in turn (module docstring):
    the slot carries the bits numpy gives for the planted entry, which beats the rest of the state"""
    import torch
    with layer(name) as S:
        B, P = S.B, S.P
        big_facts(name, S)
        st_h = P["state"]
        st = tuple(dev(a) for a in st_h)
        r, c = dev(P["r"]), dev(P["c"])
        poison = tuple(np.full(S.ncon, NAN) for _ in range(3))
        sol_h = np.random.default_rng(21).standard_normal(S.n)
        sol = dev(sol_h)
        base_alpha = bref.step(B, st_h, sol_h, poison)[1]
        keep = [t.clone() for t in st]

        def alpha_at(i, value, x_value=None):
            """barrier_step with sol[i] = value (and the point's entry i = x_value): the device's two step lengths, numpy's on the cut"""
            B1, st1, iv, ir = cut_at(S, st_h, i)
            st1 = [a.copy() for a in st1]
            sol1 = np.array([value])
            vec = 0 if i < S.nvar else 1
            j = i if i < S.nvar else i - S.nvar
            if x_value is not None:
                st1[vec][0] = x_value
                st[vec][j] = x_value
            sol[i] = value
            dirs, alpha = step(S, st, sol)
            # on the cut of one row sol = [dy], of one variable sol = [dx]
            got, one = host(alpha, 2), bref.step(B1, tuple(st1), sol1, tuple(np.full(len(ir), NAN) for _ in range(3)))[1]
            return got, np.minimum(base_alpha, one), one, dirs, alpha

        def restore(i):
            sol[i] = float(sol_h[i])
            for t, k in zip(st, keep):
                t.copy_(k)

        for slot, what in ((0, "alpha_primal"), (1, "alpha_dual")):
            for label, i in planted(S, "lower"):
                value = -1e9 if slot == 0 else 1e9      # towards a lower bound: the primal step; away from it: dz < 0, the dual step
                got, want, one, _, _ = alpha_at(i, value)
                print(f"{name} {what} planted at {label}: {got.tolist()}, the entry alone {one.tolist()}, the rest {base_alpha.tolist()}")
                assert one[slot] < base_alpha[slot] and same_bits(got, want), (what, label, got, want)
                restore(i)
        for label, i in planted(S, "lower"):
            # a NaN direction; a point exactly on its relaxed bound with a direction through it: alpha_p = +0.0, update moves nothing
            j = i if i < S.nvar else i - S.nvar
            bound = float((B["xl"] if i < S.nvar else B["rl"])[j])
            for case, value, x_value in (("NaN direction", NAN, None), ("on its bound", -1.0 if i < S.nvar else -1e9, bound)):
                got, want, one, dirs, alpha = alpha_at(i, value, x_value)
                print(f"{name} {case} at {label}: alpha {got.tolist()}")
                assert same_bits(got[:1], [0.0]) and same_bits(one[:1], [0.0]) and same_bits(got, want), (case, label, got, one)
                before = [t.clone() for t in st]
                update(S, st, sol, dirs, alpha)
                assert all(torch.equal(a.view(torch.int64), b_.view(torch.int64)) for a, b_ in zip(st, before)), (case, label)
                restore(i)
        # the four maxima: r (a variable), y (an inequality row), c (a row), a multiplier (an entry with a lower bound)
        base = bref.error(B, st_h, P["r"], P["c"])[0]
        assert same_bits(host(error(S, st, r, c), 8)[:4], base)
        r_h, c_h = P["r"], P["c"]
        for slot, what, kind in ((0, "r", "variable"), (1, "y", "inequality row"), (2, "c", "row"), (3, "z", "lower")):
            for label, i in planted(S, kind):
                B1, st1, iv, ir = cut_at(S, st_h, i)
                st1 = [a.copy() for a in st1]
                r1, c1 = r_h[iv].copy(), c_h[ir].copy()
                j = i if i < S.nvar else i - S.nvar
                vec, host_vec = {"r": (r, r1), "y": (st[2], st1[2]), "c": (c, c1), "z": (st[3], st1[3]) if i < S.nvar else (st[5], st1[5])}[what]
                old = float(vec[j])
                vec[j] = 1e30
                host_vec[0] = 1e30
                got = host(error(S, st, r, c), 8)[:4]
                one = bref.error(B1, tuple(st1), r1 if len(iv) else None, c1)[0]
                want = np.maximum(base, np.where(np.isnan(one), 0.0, one))      # (a cut without variables has no out[0])
                print(f"{name} out[{slot}] planted ({what}) at {label}: {got.tolist()}")
                assert one[slot] > base[slot] and same_bits(got, want), (what, label, got, want)
                vec[j] = old
        assert same_bits(host(error(S, st, r, c), 8)[:4], base)


def check_sums(name, S, out, st_h, c_h, logs):
    """out[4..6] are the bits of the restatement in the device's order on the object's own grid; out[7] (the device's log) lies within
    sum_bound of the same order over numpy's logs, and of math.fsum"""
    n_wg = S.info["workgroups"]
    assert n_wg == min(-(-S.n // 256), 4096)
    want = bref.error_sums(S.B, st_h, c_h, n_wg)
    print(name, "workgroups", n_wg, "out[4..7]", out[4:8].tolist(), "device order", want.tolist())
    assert same_bits(out[4:7], want[:3]), (out[4:7], want[:3])
    fs, bound = bref.sum_bound(logs)
    print(name, f"out[7] = {out[7]!r}, device order over numpy's logs {want[3]!r}, fsum {fs!r}, bound {bound:.3e}, terms {len(logs)}")
    assert abs(out[7] - want[3]) <= bound and abs(out[7] - fs) <= bound


def _solver(S, mode):
    k = C.c_void_p()
    S.check(S.L.iem_kkt_create(S.gm._h, 0, C.byref(k)))
    S.check(S.L.iem_kkt_set_border(k, mode))
    return k


def _iteration(S, k, st, bufs, asynchronous):
    """evaluation -> terms -> assemble -> factor -> refined solve (one step) -> step; with `asynchronous` also update and error"""
    c, r, obj, jv, hv, sigma, dcon, rhs, sol, dirs, alpha, out, inertia = bufs
    S.gm.eval_residual(st[0][:S.nvar], st[2][:S.ncon], 1.0, c=c[:S.ncon], out=r[:S.nvar], obj=obj)
    S.gm.jac_hess_coord(st[0][:S.nvar], st[2][:S.ncon], jv, hv, obj_weight=1.0)
    S.gm._sync_stream()
    S.check(S.L.iem_barrier_terms(S.b, *map(_p, st), _p(r), _p(c), MU, _p(sigma), _p(dcon), _p(rhs)))
    S.check(S.L.iem_kkt_assemble_diag(k, _p(hv), _p(jv), _p(sigma), _p(dcon), DW, DC))
    if asynchronous:
        S.check(S.L.iem_kkt_factor_async(k, _p(inertia)))
    else:
        got = (C.c_int64 * 3)()
        S.check(S.L.iem_kkt_factor(k, got))
        inertia.copy_(inertia.new_tensor(list(got)))
    S.check(S.L.iem_kkt_solve_refined_diag(k, _p(st[0]), _p(st[2]), 1.0, _p(sigma), _p(dcon), DW, DC, 1, _p(rhs), S.n, _p(sol), S.n, 1, None))
    S.check(S.L.iem_barrier_step(S.b, *map(_p, st), _p(sol), MU, TAU, *map(_p, dirs), _p(alpha)))
    if asynchronous:
        S.check(S.L.iem_barrier_update(S.b, *map(_p, st), _p(sol), *map(_p, dirs), _p(alpha), MU, KAPPA))
        S.check(S.L.iem_barrier_error(S.b, *map(_p, st), _p(r), _p(c), MU, _p(out)))


def _buffers(S):
    import torch
    meta = S.gm.meta
    return (nan(S.ncon), nan(S.nvar), nan(1)[:1], nan(int(meta.nnzj))[:int(meta.nnzj)], nan(int(meta.nnzh))[:int(meta.nnzh)], nan(S.nvar), nan(S.ncon), nan(S.n), nan(S.n),
            tuple(nan(q) for q in S.dsizes), nan(2), nan(8), torch.zeros(3, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("name,mode", [("opf_7", 1), ("pandemic_20x3", 0)])
def test_through_the_solver_object(name, mode, built):
    """the device directions satisfy the unreduced Newton system (oracle matrices on the host) within ten times the residual the
    numpy + scipy path reaches on the same inputs, measured in the run, floor 1e-15·scale (the rule of test_kkt_object)"""
    from scipy.sparse.linalg import splu
    with layer(name) as S:
        B, P, om = S.B, S.P, S.P["om"]
        k = _solver(S, mode)
        try:
            st = tuple(dev(a) for a in P["state"])
            bufs = _buffers(S)
            _iteration(S, k, st, bufs, False)
            c, r, _, _, _, sigma, dcon, rhs, sol, dirs, alpha, _, inertia = bufs
            assert tuple(inertia.tolist()) == (S.nvar, S.ncon, 0), inertia.tolist()
            sol_d = host(sol, S.n)
            dirs_d = tuple(host(g, q) for g, q in zip(dirs, S.dsizes))
            # the host path on the same inputs
            sg, dcn, rh = bref.terms(B, P["state"], P["r"], P["c"])
            K = dref.host_kkt_diag(om, P["state"][0], P["state"][2], sg, DW, dcn + DC)
            sol_h = splu(K.tocsc()).solve(rh)
            dirs_h, _ = bref.step(B, P["state"], sol_h, tuple(np.full(S.ncon, NAN) for _ in range(3)))
            WJ = bref.oracle_matrices(om, P["state"][0], P["state"][2])
            worst = lambda s_, d_: max(float(np.abs(b).max()) if b.size else 0.0 for b in bref.newton_blocks(P, WJ, s_, d_, DW, DC))
            scale = max(1.0, np.abs(rh).max(), np.abs(sol_h).max())
            own, got = worst(sol_h, dirs_h), worst(sol_d, dirs_d)
            bound = 10.0 * max(own, 1e-15 * scale)
            print(f"{name}: delta_w {DW}, inertia {inertia.tolist()}, scale {scale:.3e}, numpy + scipy residual {own:.3e}, device residual {got:.3e} (bound {bound:.3e}), alpha {host(alpha, 2).tolist()}")
            assert got <= bound
        finally:
            S.check(S.L.iem_kkt_destroy(k))


@pytest.mark.parametrize("name,mode", [("pandemic_20x3", 1), ("opf_7", 1)])
def test_one_iteration_in_one_graph(name, mode, built):
    """evaluation, terms, assemble, factor (async), refined solve, step, update, error captured once on the handle's stream — a linear
    chain — and replayed from two starting states copied into the same buffers: each replay bitwise the eager sequence from that state"""
    import torch
    with layer(name) as S:
        k = _solver(S, mode)
        try:
            states = [bref.barrier_point(name, seed)["state"] for seed in (0, 1)]
            st = tuple(nan(q) for q in S.sizes)
            bufs = _buffers(S)
            results = lambda: [t.clone() for t in st] + [bufs[8].clone(), bufs[10].clone(), bufs[11].clone(), bufs[12].clone()] + [t.clone() for t in bufs[9]]

            def load(which):
                for t, a in zip(st, states[which]):
                    t[:len(a)] = torch.from_numpy(a)
                for t in (bufs[8], bufs[10], bufs[11]) + bufs[9]:
                    t.fill_(NAN)
                bufs[12].zero_()
            eager = []
            for which in (1, 0):      # (the first eager sequence does the set-up)
                load(which)
                _iteration(S, k, st, bufs, True)
                torch.cuda.synchronize()
                eager.append(results())
            eager = eager[::-1]
            assert not torch.equal(eager[0][0], eager[1][0])
            assert eager[0][-6].tolist() == [S.nvar, S.ncon, 0] and float(eager[0][8][0]) > 0.0
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                _iteration(S, k, st, bufs, True)
            S.gm._sync_stream()
            for which in (0, 1, 0):
                load(which)
                g.replay()
                torch.cuda.synchronize()
                for a, b in zip(results(), eager[which]):
                    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), which
        finally:
            S.check(S.L.iem_kkt_destroy(k))


def test_refusals_and_the_python_layer(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import BarrierLayer
    from infiniteexamodels.jl_amd.model import ExaModel
    with layer("opf_7") as S:
        B, P, L = S.B, S.P, S.L
        err = lambda: L.iem_last_error().decode()
        st = tuple(dev(a) for a in P["state"])
        r, c, sol = dev(P["r"]), dev(P["c"]), dev(np.random.default_rng(21).standard_normal(S.n))
        dirs, alpha = step(S, st, sol)
        before = state_host(S, st)
        assert L.iem_barrier_step(S.b, *map(_p, st), _p(sol), MU, 1.5, *map(_p, dirs), _p(alpha)) == -4 and "tau" in err()
        assert L.iem_barrier_step(S.b, *map(_p, st), None, MU, TAU, *map(_p, dirs), _p(alpha)) == -4 and "null" in err()
        assert L.iem_barrier_update(S.b, *map(_p, st), _p(sol), *map(_p, dirs), _p(alpha), MU, 0.5) == -4 and "kappa_sigma" in err()
        assert L.iem_barrier_update(S.b, *map(_p, st), _p(sol), *map(_p, dirs), _p(alpha), -1.0, KAPPA) == -4 and "mu" in err()
        assert L.iem_barrier_error(S.b, *map(_p, st), _p(r), _p(c), MU, None) == -4 and "null" in err()
        assert L.iem_barrier_terms(S.b, *map(_p, st[:1]), None, *map(_p, st[2:]), _p(r), _p(c), MU, _p(nan(S.nvar)), _p(nan(S.ncon)), _p(nan(S.n))) == -4 and "null" in err()
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip(state_host(S, st), before))      # a refused call does no device work
        bad = P["lvar"].copy(); bad[0] = np.inf
        out = C.c_void_p()
        assert L.iem_barrier_create(S.gm._h, bad.ctypes.data, None, None, None, 1e-8, C.byref(out)) == -4 and "lvar > uvar" in err()
        assert L.iem_barrier_create(S.gm._h, None, None, None, None, 0.0, C.byref(out)) == -4 and "fixed" in err()
        assert L.iem_barrier_create(S.gm._h, None, None, None, None, -1.0, C.byref(out)) == -4 and "relax" in err()
        # BarrierLayer against the raw calls, bitwise
        with BarrierLayer(S.gm, relax=bref.RELAX) as bar:
            assert {q: bar.info[q] for q in B["counts"]} == B["counts"] and bar.info["workgroups"] == S.info["workgroups"]
            T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            ts = tuple(T(a) for a in P["state"])
            tr, tc, tsol = T(P["r"]), T(P["c"]), sol[:S.n].clone()
            for a, b_, q in zip(bar.terms(ts, tr, tc, MU), terms(S, st, r, c), (S.nvar, S.ncon, S.n)):
                assert same_bits(a.cpu().numpy(), host(b_, q))
            tdirs, talpha = bar.step(ts, tsol, MU, TAU, out=tuple(torch.full((q,), NAN, dtype=torch.float64, device="cuda") for q in S.dsizes))
            for a, b_, q in zip(tdirs + (talpha,), dirs + (alpha,), S.dsizes + (2,)):
                assert same_bits(a.cpu().numpy(), host(b_, q))
            assert talpha.is_cuda and talpha.shape == (2,)
            e = bar.error(ts, tr, tc, MU)
            assert e.is_cuda and same_bits(e.cpu().numpy(), host(error(S, st, r, c), 8))
            assert same_bits(bar.merit(ts[0], ts[1], tc).cpu().numpy(), e[6:8].cpu().numpy())
            assert same_bits(bar.error(ts, None, tc, MU)[1:].cpu().numpy(), e[1:].cpu().numpy())
            E = BarrierLayer.optimality_error(e, (bar.info["ncon"], bar.info["nz"]))
            assert E[0] == max(E[1:]) and E[2] == float(e[2]) and all(v >= 0 for v in E)
            assert bar.update(ts, tsol, tdirs, talpha, MU) is ts
            update(S, st, sol, dirs, alpha)
            for a, b_ in zip(ts, state_host(S, st)):
                assert same_bits(a.cpu().numpy(), b_)
            x0 = T(P["om"].x0)
            raw_x = dev(P["om"].x0)
            outs = [nan(q) for q in (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)]
            S.check(L.iem_barrier_start(S.b, _p(raw_x), _p(c), *map(_p, outs), bref.PUSH, bref.FRAC))
            poisoned = tuple(torch.full((q,), NAN, dtype=torch.float64, device="cuda") for q in (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon))
            new = bar.start(x0, tc, out=poisoned)
            assert new[0] is x0 and bool((new[2] == 0).all())
            for a, b_, q in zip((new[0], new[1], new[3], new[4], new[5], new[6]), [raw_x] + outs, (S.nvar, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)):
                assert same_bits(a.cpu().numpy(), host(b_, q))
            # what ExaModel's methods reject: a non-contiguous tensor, another length, another dtype
            with pytest.raises(ValueError, match="contiguous"):
                bar.terms((torch.stack([ts[0], ts[0]], dim=1)[:, 0],) + ts[1:], tr, tc, MU)
            with pytest.raises(ValueError):
                bar.terms(ts, tr[:-1], tc, MU)
            with pytest.raises(ValueError):
                bar.step(ts, tsol.float(), MU, TAU)
            with pytest.raises(iemlib.IemError, match="tau"):
                bar.step(ts, tsol, MU, 0.0)
        with pytest.raises(iemlib.IemError, match="closed"):
            bar.merit(ts[0], ts[1], tc)
    # a sharded handle holds one rank's window
    sm = ExaModel.sharded(bref.barrier_point("quadrotor_100")["blob"], 1, 0, 2, device=0)
    try:
        with pytest.raises(iemlib.IemError, match="sharded"):
            BarrierLayer(sm)
    finally:
        sm.close()
