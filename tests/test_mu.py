"""The barrier parameter object's arithmetic without a GPU: tests/mu_reference.py (the numpy restatement of csrc/iem_mu_device.h)
against tests/barrier_reference.py and a plain Python loop.

(a) the closed form: for products p >= 0 rounding is monotone, so max_i fl|p_i − mu| is bitwise max(fl(p_max − mu), fl(mu − p_min)) —
    what lets ONE kernel run the Fiacco–McCormick loop from two extremes;
(b) `update` against a transcription of the loop of tests/search_loop.py that re-evaluates barrier_reference.error and
    BarrierLayer.optimality_error at every mu, on every branch;
(c) a model without any bound: e_c = 0, word 8 stays +inf."""
import numpy as np
import pytest

import barrier_reference as bref
import mu_reference as mref
import soc_reference

MODELS = ["opf_7", "farmer_5", "pandemic_20x3"]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def word_vector(P, st):
    """the twelve words with the sums in numpy's order (any one order serves the CPU tests)"""
    head, sums, w8, w10, p = mref.error_words(P["B"], st, P["r"], P["c"])
    return np.array([*head, *(float(np.sum(t)) for t in sums), w8, float(np.sum(p)), w10, 0.0])


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_closed_form_of_the_complementarity_maximum(name, seed, built):
    P = bref.barrier_point(name, seed)
    B, st = P["B"], P["state"]
    head, _, w8, w10, p = mref.error_words(B, st, P["r"], P["c"])
    assert w10 == 0.0 and (p > 0).all() and w8 == p.min() and head[3] == p.max()
    pmax, pmin = np.float64(head[3]), np.float64(w8)
    mus = [0.0, 5e-324, 1e-11, 0.1, pmax, pmin, np.nextafter(pmax, 0), np.nextafter(pmax, np.inf), np.nextafter(pmin, 0), np.nextafter(pmin, np.inf),
           float(np.median(p)), 1e9]
    for mu in mus:
        mu = np.float64(mu)
        want = bref.error(B, st, P["r"], P["c"], float(mu))[0][3]
        got = np.maximum(pmax - mu, mu - pmin)
        assert bits(got) == bits(want), (name, seed, float(mu), float(got), float(want))


def host_loop(P, st, blk, opts):
    """the loop of tests/search_loop.py, word for word but for mu·sqrt(mu): (mu, tau, decreases, status, flag)"""
    from infiniteexamodels.jl_amd.barrier import BarrierLayer
    B = P["B"]
    counts = (B["counts"]["ncon"], B["counts"]["nz"])

    def err(mu):
        head, ay, mult, theta, logs = bref.error(B, st, P["r"], P["c"], mu)
        return BarrierLayer.optimality_error([*head, float(np.sum(ay)), float(np.sum(mult)), float(np.sum(theta)), float(np.sum(logs))], counts)[0]
    mu, tau = float(blk[0]), float(blk[1])
    p = mref.products(B, st)
    e0 = err(0.0)
    if (~mref.enters(p)).any() or np.isnan(e0):
        return mu, tau, 0, mref.UNUSABLE, 0
    if e0 <= opts["tol"]:
        return mu, tau, 0, mref.CONVERGED, 0
    k = 0
    while mu > opts["mu_floor"] and err(mu) <= opts["kappa_eps"] * mu and k < 64:
        mu = max(opts["mu_floor"], min(opts["kappa_mu"] * mu, mu * float(np.sqrt(mu))))
        k += 1
    if k:
        tau = max(opts["tau_min"], 1.0 - mu)
    return mu, tau, k, mref.ITERATING, int(k > 0)


@pytest.mark.parametrize("name", MODELS)
def test_update_is_the_host_loop(name, built):
    seen = {}
    for label, P, st, blk, opts, want in mref.branch_cases(name):
        counts = (P["B"]["counts"]["ncon"], P["B"]["counts"]["nz"])
        w = word_vector(P, st)
        ctl = np.arange(16, dtype=np.float64) + 1.0
        new, ctl2 = mref.update(blk, w, counts, opts, ctl)
        iw = mref.ints(new)
        mu, tau, k, status, flag = host_loop(P, st, blk, opts)
        assert bits(new[0]) == bits(mu) and bits(new[1]) == bits(tau), (label, new[0], mu)
        assert (iw[10], iw[8], iw[9] & 1, iw[11]) == (k, status, flag, 1), (label, iw[8:12], k, status)
        assert bits(new[2]) == bits(np.sqrt(np.float64(mu))) or k == 0
        assert (ctl2[11] == 0.0 and ctl2[12] == 0.0) == (k > 0) and np.array_equal(np.delete(ctl2, [11, 12]), np.delete(ctl, [11, 12]))
        if want == ">=3":
            assert k >= 3, (label, k)
        elif want is not None:
            assert k == want, (label, k)
        seen[label] = (k, status, float(mu))
    assert seen["converged"][1] == mref.CONVERGED and seen["a NaN multiplier"][1] == mref.UNUSABLE and seen["a negative product"][1] == mref.UNUSABLE
    assert seen["stop at the floor"][2] == 1e-10 and seen["stop at the floor"][0] >= 1
    assert seen["far from the path"][1] == mref.ITERATING and seen["one decrease"][1] == mref.ITERATING


def test_a_cleared_flag_and_the_counters(built):
    """a second update without a decrease clears flag bit 0 and keeps the count of decreases"""
    label, P, st, blk, opts, _ = mref.branch_cases("opf_7")[2]
    counts = (P["B"]["counts"]["ncon"], P["B"]["counts"]["nz"])
    one, _ = mref.update(blk, word_vector(P, st), counts, opts)
    k = int(mref.ints(one)[10])
    assert k >= 3 and mref.ints(one)[9] == 1
    P0 = bref.barrier_point("opf_7")
    two, _ = mref.update(one, word_vector(P0, P0["state"]), counts, opts)
    assert tuple(mref.ints(two)[8:12]) == (mref.ITERATING, 0, k, 2) and bits(two[0]) == bits(one[0])
    again = mref.reset(two, opts, 0.5)
    assert tuple(mref.ints(again)[8:12]) == (0, 0, 0, 0) and again[0] == 0.5 and again[1] == 0.99 and bits(again[3:8]).tolist() == bits(two[3:8]).tolist()


def test_no_bounds_no_complementarity(built):
    P = soc_reference.maratos_point()
    B = P["B"]
    assert B["counts"]["nz"] == 0
    w = word_vector(P, P["state"])
    assert w[8] == np.inf and w[3] == 0.0 and w[9] == 0.0 and w[10] == 0.0
    counts = (B["counts"]["ncon"], 0)
    opts = mref.options()
    e_d, e_p, sc = mref.terms(w, counts, opts)
    for mu in (0.0, 0.1, 1e9):
        assert mref.e_c(w, counts, sc, np.float64(mu)) == 0.0
    blk, _ = mref.update(mref.fresh_block(opts), w, counts, opts)
    assert blk[7] == 0.0 and bits(blk[3]) == bits(np.maximum(e_d, e_p)) and mref.ints(blk)[8] == mref.ITERATING


def test_the_bound_barrier_object_is_the_barrier_text_with_four_reads_moved(built):
    """iem_barrier_bind_mu loads a variant DERIVED from the barrier object's text: the unbound object keeps its source (its key is pinned
    in tests/golden/kkt_source_keys.json), and the variant differs from it in the Args struct and the one read per kernel only"""
    import difflib
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.barrier_source()
    bound, bkey = iemlib.barrier_mu_source()
    assert bkey != key and iemlib.barrier_mu_source() == (bound, bkey)
    gone, new = [], []
    for line in difflib.unified_diff(src.split("\n"), bound.split("\n"), lineterm="", n=0):
        if line.startswith("-") and not line.startswith("---"):
            gone.append(line[1:].strip())
        elif line.startswith("+") and not line.startswith("+++"):
            new.append(line[1:].strip())
    assert gone == ["const double mu = A.mu;", "const double mu = A.mu, tau = A.tau, ntau = -A.tau;", "const double mu = A.mu, kappa = A.kappa;", "const double mu = A.mu;"], gone
    assert new == ["const double *mu_blk;      // the iem_mu block {mu, tau, ...}", "const double mu = A.mu_blk[0];",
                   "const double mu = A.mu_blk[0], tau = A.mu_blk[1], ntau = -tau;", "const double mu = A.mu_blk[0], kappa = A.kappa;", "const double mu = A.mu_blk[0];"], new
    assert "A.mu " not in bound.split("// iem_barrier_device.h", 1)[1].replace("A.mu_blk", "") and "A.tau" not in bound
