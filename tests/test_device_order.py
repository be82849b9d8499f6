"""The order-aware sums of the restatements without a GPU: every parked column that tests/test_gpu_{barrier,search,resto,mu,amu}.py
compare bit for bit — barrier_reference.error_addends, search_reference.slope_addends, resto_reference.merit_addends /
slope_addends / error_addends, mu_reference.product_addends, amu_reference.probe_addends — through barrier_reference.device_sum.

(a) one workgroup with one populated lane: device_sum is the plain loop over that lane's entries, addend after addend;
(b) at both big shapes (quadrotor(27 000) and quadrotor(60 000) of barrier_reference.big_point, 4096 workgroups) the device-order
    value lies within barrier_reference.sum_bound of math.fsum of the COMPACT term lists the older tests use: the padded layout is
    tied to them, and the inputs keep the restatement itself inside every bound the GPU tests retain;
(c) the inputs discriminate: at the 60 000 shape, adding upper before lower inside an entry and accumulating the trips last-to-first
    each change the bits of every column they can reach (a column with one addend per entry has no upper and lower to swap)."""
import numpy as np
import pytest

import amu_reference as aref
import barrier_reference as bref
import mu_reference as mref
import resto_reference as rref
import search_reference as sref

SHAPES = [27_000, 60_000]
_cols = {}


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def columns(supports):
    """``[(label, addends, compact terms)]`` of every new order-aware sum at big_point(supports), built once per size"""
    if supports in _cols:
        return _cols[supports]
    P = bref.big_point(supports)
    B, st = P["B"], P["state"]
    x, s = st[0], st[1]
    nvar, ncon = len(x), len(st[2])
    out = []
    _, ay, mult, theta, logs = bref.error(B, st, P["r"], P["c"])
    for label, col, terms in zip(("barrier |y|", "barrier multipliers", "barrier theta", "barrier log gap"), bref.error_addends(B, st, P["c"]), (ay, mult, theta, logs)):
        out.append((label, col, terms))
    g, hs, hds, _, _ = sref.big_inputs(supports)
    out.append(("search slope", sref.slope_addends(B, x, s, g, hs, hds, bref.MU), sref.slope_terms(B, x, s, g, hs, np.where(B["eq"], 0.0, hds), bref.MU)))
    E = rref.big_entered(supports)
    R, est = E["R_step"], E["state"]
    for label, col, terms in zip(("resto S0", "resto S1", "resto theta_R", "resto L"), rref.merit_addends(B, R, 0, est[0], est[1], P["c"]),
                                 rref.merit_terms(B, R, 0, est[0], est[1], P["c"])):
        out.append((label, col, terms))
    out.append(("resto slope", rref.slope_addends(B, R, est, E["sol"], E["dirs"][0], E["mu"], E["zeta"]),
                rref.slope_terms(B, R, est, E["sol"], np.where(B["eq"], 0.0, E["dirs"][0]), E["mu"], E["zeta"])))
    _, ay, mult, _, _ = rref.error(B, R, est, P["r"], P["c"], E["mu"], E["zeta"])
    cols = rref.error_addends(B, R, est, P["c"])
    out += [("resto |y|", cols[0], ay), ("resto multipliers", cols[1], mult)]
    (pL, pU), _ = mref.product_addends(B, st)
    out.append(("mu products", [pL, pU], mref.products(B, st)))
    asol, dirs, alpha = aref.directions(P)
    out.append(("amu probe", list(aref.probe_addends(B, st, asol, dirs, alpha)), aref.probe_terms(B, st, asol, dirs, alpha)))
    _cols[supports] = out
    return out


def last_to_first(addends, n_wg):
    """device_sum with ONE fault: a lane accumulates its trips in the reverse order"""
    T = 256 * n_wg
    n = len(addends[0])
    pad = -(-n // T) * T
    rev = []
    for a in addends:
        b = np.zeros(pad)
        b[:n] = a
        rev.append(b.reshape(-1, T)[::-1].reshape(-1))
    return bref.device_sum(rev, n_wg)


def test_one_populated_lane_is_the_plain_loop():
    """lane 37 of ONE workgroup, five trips: what device_sum gives is the loop `for trip: for addend: acc += addend[entry]`"""
    lane, n = 37, 256 * 5 - 100      # (a ragged last trip: the lane's fifth entry exists, the tail of the workgroup does not)
    nvar = bref.big_point(27_000)["B"]["counts"]["nvar"]
    for label, col, _ in columns(27_000):
        cut = []
        for a in col:
            keep = a[nvar - n // 2:][:n]      # a window across the nvar seam: both branches where the column has both
            b = np.zeros(n)
            b[lane::256] = keep[lane::256]
            cut.append(b)
        acc = np.float64(0.0)
        for k in range(lane, n, 256):
            for b in cut:
                acc = acc + b[k]
        assert len(range(lane, n, 256)) == 5 and acc != 0.0, label
        assert bits(bref.device_sum(cut, 1)) == bits(acc), label


@pytest.mark.parametrize("supports", SHAPES)
def test_device_order_within_the_bound_of_fsum(supports):
    P = bref.big_point(supports)
    cn = P["B"]["counts"]
    n = cn["nvar"] + cn["ncon"]
    n_wg = bref.grid(n)
    trips = bref.trips(cn["nvar"], n, n_wg)
    print(f"quadrotor({supports}): n {n}, workgroups {n_wg}, trips {len(trips)}, (variables, rows) per trip {trips}")
    assert n_wg == 4096 and sum(a + b for a, b in trips) == n
    if supports == 60_000:
        assert (cn["nvar"], cn["ncon"], n) == (1_320_000, 1_080_000, 2_400_000) and cn["nvar"] > 2 ** 20
        assert len(trips) == 3 and trips[0][1] == 0 and trips[1][0] > 0 and trips[1][1] > 0 and trips[2][0] == 0
    else:
        assert n == 1_080_000 and cn["nvar"] < 2 ** 20 and len(trips) == 2 and trips[1][0] == 0
    for label, col, terms in columns(supports):
        got = float(bref.device_sum(col, n_wg))
        want, bound = bref.sum_bound(terms)
        assert all(len(a) == n for a in col), label
        assert sum(int(np.count_nonzero(a)) for a in col) == int(np.count_nonzero(terms)), label      # the padded layout holds the compact terms
        ulp = abs(got - want) / np.spacing(abs(want))
        print(f"  {label}: device order {got!r}, fsum {want!r}, {ulp:.1f} ulp apart, bound {bound / np.spacing(abs(want)):.3g} ulp")
        assert abs(got - want) <= bound, label


def misordered(supports):
    """``(the faults that did NOT change the bits, the columns whose trips could show)`` at big_point(supports)"""
    P = bref.big_point(supports)
    cn = P["B"]["counts"]
    n = cn["nvar"] + cn["ncon"]
    n_wg = bref.grid(n)
    T = 256 * n_wg
    same, reached = [], []
    for label, col, _ in columns(supports):
        want = bref.device_sum(col, n_wg)
        # a lane whose trips hold at most two non-zero addends adds them commutatively: no order of the trips can show.  That is every
        # column that lives on rows alone (the rows of this shape lie on the second and third trip), whatever the seed
        per_lane = sum(np.count_nonzero(np.pad(a, (0, 3 * T - n)).reshape(3, T), axis=0) for a in col)
        if per_lane.max() >= 3:
            reached.append(label)
            if bits(last_to_first(col, n_wg)) == bits(want):
                same.append((label, "trips last-to-first"))
        else:
            assert all(not a[:cn["nvar"]].any() for a in col), label
        if len(col) > 1 and bits(bref.device_sum(col[::-1], n_wg)) == bits(want):
            same.append((label, "upper before lower"))
    return same, reached


def test_misorderings_change_the_bits():
    """Every column but the sums of logs, which the GPU tests hold to a tolerance (the device's log) and whose addends (|log gap| <
    750) cannot outweigh a total of 10⁶: they are reported, not asserted."""
    same, reached = misordered(60_000)
    print("trips last-to-first can show in:", reached)
    print("no change of bits:", same)
    assert set(reached) == {"barrier multipliers", "barrier log gap", "search slope", "resto S1", "resto L", "resto slope", "resto multipliers", "mu products", "amu probe"}
    assert not [f for f in same if f[0] not in ("barrier log gap", "resto L")], same
