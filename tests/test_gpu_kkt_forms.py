"""Every chain KKT kernel form of tests/cases_kkt_forms.py on the MI355X, through iem_kkt_chain_factor / _solve / _solve_many /
_level / _solve_lanes on a small ExaModel handle.

Per case: the pivot counts, D^-1 (Z, Gp) block by block against tests/chain_reference.py, the solution against the refined dense
solution x_ref, iem_kkt_chain_solve_many with KKT_MR + 1 columns (one full chunk and a one-column remainder) bit for bit against
the single-column solves, and a 64-double tail behind every device array that nobody may have touched.

Tolerance: 16 max(err_cpu, n 2^-52) per column, err_cpu being the restatement's own distance from x_ref in the same run (the
device does the restatement's eliminations with sums grouped differently); never derived from device output.  The factors
are held to the bound of column 0.  Measured figures per case: profiles/kkt_forms.json."""
import ctypes as C
import json

import numpy as np
import pytest

import cases_kkt_forms as kf

pytestmark = pytest.mark.gpu
TAIL = 64
PATTERN = 0x7FF4C0DEC0DE5EED      # a signalling-NaN bit pattern no kernel produces
RESULTS = {}


class Dev:
    """Device arrays with a tail: `new(name, host array)` uploads, `check()` compares every tail (and every read-only array) afterwards."""

    def __init__(self):
        import torch
        self.torch, self.arrays, self.const = torch, {}, {}

    def new(self, name, a, const=False):
        torch = self.torch
        a = np.ascontiguousarray(a)
        words = 8 // a.dtype.itemsize
        t = torch.empty(a.size + TAIL * words, dtype=getattr(torch, a.dtype.name), device="cuda")
        t[:a.size] = torch.from_numpy(a.ravel())
        t[a.size:].view(torch.int64).fill_(PATTERN)
        self.arrays[name] = (t, a.size, a.shape)
        if const:
            self.const[name] = a.copy()
        return t

    def ptr(self, name, offset=0):
        t = self.arrays[name][0]
        return C.c_void_p(t.data_ptr() + offset * t.element_size())

    def get(self, name):
        t, n, shape = self.arrays[name]
        return t[:n].cpu().numpy().reshape(shape)

    def check(self, where):
        for name, (t, n, shape) in self.arrays.items():
            tail = t[n:].view(self.torch.int64).cpu().numpy()
            assert (tail == PATTERN).all(), (where, "written past the end of", name, np.flatnonzero(tail != PATTERN)[:8])
        for name, a in self.const.items():
            assert np.array_equal(self.get(name), a), (where, "a read-only array changed", name)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _level_of(i, T):
    t = i % T
    return "last block" if t == 0 else "level s = %d" % (t & -t)


def _per_block(what, got, want, bound, T):
    """max |got - want| / max(1, max |want|) over all blocks, and the block (with its level) where it is largest."""
    if want.size == 0:
        return 0.0
    scale = max(1.0, np.abs(want).max())
    err = np.abs(got - want).reshape(want.shape[0], -1).max(axis=1) / scale
    err = np.where(np.isfinite(err), err, np.inf)
    worst = int(err.argmax())
    assert err[worst] <= bound, "%s: block %d (%s) differs by %.3e, bound %.3e; blocks beyond it: %s" % (
        what, worst, _level_of(worst, T), err[worst], bound, np.flatnonzero(err > bound)[:16].tolist())
    return float(err[worst])


@pytest.fixture(scope="module")
def handle(built):
    from infiniteexamodels.jl_amd import transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(transcribe.exa_core(workloads.quadrotor(10)), device=0)
    yield gm
    gm.close()


@pytest.mark.parametrize("case_id", [c.id for c in kf.CASES])
def test_form(case_id, handle):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    gm, L = handle, handle._L
    c, d, r = kf.BY_ID[case_id], kf.data(case_id), kf.reference(case_id)
    nb, ne, nc = c.shape
    S, T, n = c.S, c.T, c.n
    form = next(f for f in kf.FORMS if f["shape"] == c.shape)
    nrhs = form["defs"]["mr"] + 1
    assert nrhs <= kf.NRHS_MAX
    chained, laned = c.kind != "unchained", c.kind == "laned"
    Bt0 = d.Bt.copy()
    Bt0[::T] = d.junk      # no block to the left of a lane's first: whatever sits there is never read
    dev = Dev()
    dev.new("D", d.D); dev.new("Bt", Bt0); dev.new("BR", np.zeros((S, nc, nc))); dev.new("E", d.E if ne else np.zeros(1))
    dev.new("Z", np.zeros((S, nb, max(ne, 1)))); dev.new("Gp", np.zeros((S, max(ne, 1), max(ne, 1)))); dev.new("info", np.full(4, -1, np.int64))
    dev.new("rows", d.rows, const=True); dev.new("cols", d.cols, const=True)
    p = dev.ptr
    chain = (p("Bt"), p("BR"), p("rows"), p("cols")) if chained else (None, None, None, None)
    gm._sync_stream()

    # ---- factorisation --------------------------------------------------------------------------------------------------------
    if laned:
        lvl = lambda s, what: iemlib.check(L.iem_kkt_chain_level(gm._h, S, T, nb, nc, p("D"), p("Bt"), p("BR"), p("rows"), p("cols"), p("info"), 1e-30, s, what))
        lvl(1, 3)
        s = 1
        while s < T:
            lvl(s, 0); lvl(s, 1)
            s *= 2
        lvl(1, 2)
    else:
        iemlib.check(L.iem_kkt_chain_factor(gm._h, S, nb, ne, nc, p("D"), *chain, p("E"), p("Z"), p("Gp"), p("info"), 1e-30))
    torch.cuda.synchronize()
    dev.check("factor")
    info = dev.get("info")
    assert (int(info[0]), int(info[1])) == (r.neg, 0), ("negative pivots / pivots below the threshold", info[:2].tolist(), r.neg)
    rec = dict(n=n, err_cpu=r.err_cpu, err_inv=r.err_inv, bound=r.bound)
    rec["Dinv"] = _per_block("D^-1", dev.get("D"), r.Dinv, r.bound, T)
    if ne:
        rec["Z"] = _per_block("Z", dev.get("Z"), r.Z, r.bound, T)
        rec["Gp"] = _per_block("Gp", dev.get("Gp"), r.Gp, r.bound, T)
    for name in ("D", "Bt", "BR", "Z"):      # the factors are only read from here on
        dev.const[name] = dev.get(name)

    # ---- solves: every column on its own, then all of them at once -------------------------------------------------------------------
    nep = max(ne, 0)
    Gs = d.G - dev.get("Gp")[:, :ne, :ne].sum(0) if ne else None
    fac = (p("D"), *chain, p("Z") if ne else None)
    zero_z = np.zeros((nrhs, S, nb))
    dev.new("r1", d.rhs[:nrhs]); dev.new("z1", zero_z); dev.new("rBp1", np.zeros((nrhs, S, max(ne, 1)))); dev.new("xB", np.zeros((nrhs, max(ne, 1))))
    dev.new("rm", d.rhs[:nrhs]); dev.new("zm", zero_z); dev.new("rBpm", np.zeros((nrhs, S, max(ne, 1))))

    def single(u, phase):
        # (ne = 0: rBp and xB are never touched — the planes' stride does not matter)
        args = (gm._h, S, T, nb, ne, nc, *fac, p("r1", u * S * nb), p("z1", u * S * nb) if chained else None, p("rBp1", u * S * nep) if ne else None,
                p("xB", u * nep) if ne and phase else None, phase)
        iemlib.check(L.iem_kkt_chain_solve_lanes(*args) if laned else L.iem_kkt_chain_solve(*args[:2], *args[3:]))

    def many(phase):
        iemlib.check(L.iem_kkt_chain_solve_many(gm._h, S, T if laned else 0, nb, ne, nc, *fac, p("rm"), p("zm") if chained else None, p("rBpm") if ne else None,
                                                p("xB") if ne and phase else None, nrhs, phase))

    for u in range(nrhs):
        single(u, 0)
    many(0)
    torch.cuda.synchronize()
    dev.check("forward")
    xb_errs = [0.0] * nrhs
    if ne:
        rBp1 = dev.get("rBp1")
        xB = np.stack([np.linalg.solve(Gs, d.rB[u] - rBp1[u].sum(0)) for u in range(nrhs)])      # the border system on the host, per column
        dev.arrays["xB"][0][:xB.size] = torch.from_numpy(xB.ravel()).cuda()
        dev.const["xB"] = xB.copy()
        xb_errs = [kf.rel(xB[u], r.x_ref[u][S * nb:]) for u in range(nrhs)]
        rec["xB"] = xb_errs[0]
    for u in range(nrhs):
        single(u, 1)
    many(1)
    torch.cuda.synchronize()
    dev.check("backward")
    x1, xm = dev.get("r1"), dev.get("rm")
    errs = []
    for u in range(nrhs):
        want = r.x_ref[u][:S * nb].reshape(S, nb)
        scale = max(1.0, np.abs(r.x_ref[u]).max())
        e = np.abs(x1[u] - want).max(axis=1) / scale
        e = np.where(np.isfinite(e), e, np.inf)
        worst = int(e.argmax())
        print(f"{case_id} column {u}: device {e[worst]:.3e} (block {worst}, {_level_of(worst, T)}), err_cpu {r.err_cols[u]:.3e}, bound {r.bounds[u]:.3e}")
        errs.append(float(e[worst]))
    rec["x"], rec["x_all_columns"] = errs[0], max(errs)
    rec["ratio_to_bound"] = max(max(errs[u], xb_errs[u]) / r.bounds[u] for u in range(nrhs))
    RESULTS[case_id] = rec
    for u in range(nrhs):
        assert errs[u] <= r.bounds[u], (case_id, "column", u, errs[u], r.bounds[u])
        assert xb_errs[u] <= r.bounds[u], (case_id, "border, column", u, xb_errs[u], r.bounds[u])
    # column u of the multi-column solve IS the single-column solve of it (the promise at the head of csrc/iem_kkt_many_device.h)
    for u in range(nrhs):
        assert _same_bits(xm[u], x1[u]), (case_id, "iem_kkt_chain_solve_many: column", u, "is not the single-column solve of it",
                                          float(np.abs(xm[u] - x1[u]).max()))
    if ne:
        assert _same_bits(dev.get("rBpm"), dev.get("rBp1")), (case_id, "the border terms of the multi-column forward pass")


def test_chain_calls_refuse_what_the_source_refuses(handle):
    """The shapes iem_kkt_source refuses (tests/test_kkt_forms.py) are refused by the chain calls with the same IEM_E_ARG and the
    same words, before anything is loaded or launched: the arrays (64 doubles, far too small for these shapes) keep their bits."""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    gm, L = handle, handle._L
    dev = Dev()
    dev.new("a", np.arange(64, dtype=np.float64), const=True)
    a = dev.ptr("a")
    gm._sync_stream()
    for nb, ne, nc in ((84, 68, 4), (68, 104, 4), (20, 4, 0), (22, 0, 4)):
        with pytest.raises(iemlib.IemError):
            iemlib.kkt_source(nb, ne, nc)
        words = L.iem_last_error()
        assert b"within the LDS of a CU" in words
        assert L.iem_kkt_chain_factor(gm._h, 1, nb, ne, nc, a, None, None, None, None, a, a, a, a, 1e-30) == -4 and L.iem_last_error() == words
        assert L.iem_kkt_chain_solve(gm._h, 1, nb, ne, nc, a, None, None, None, None, a, a, None, a, a, 0) == -4 and L.iem_last_error() == words
        assert L.iem_kkt_chain_solve_many(gm._h, 1, 0, nb, ne, nc, a, None, None, None, None, a, a, None, a, a, 2, 0) == -4 and L.iem_last_error() == words
    assert L.iem_kkt_chain_level(gm._h, 1, 0, 22, 4, a, a, a, a, a, a, 1e-30, 1, 0) == -4 and b"within the LDS of a CU" in L.iem_last_error()
    torch.cuda.synchronize()
    dev.check("refusals")


def test_report():
    """What the cases measured (kept in profiles/kkt_forms.json): the worst case against its bound."""
    if not RESULTS:      # (deselected cases: nothing to report)
        return
    print("KKT_FORMS_JSON " + json.dumps(RESULTS, sort_keys=True))
    worst = max(RESULTS, key=lambda k: RESULTS[k]["ratio_to_bound"])
    print("worst case against its bound:", worst, RESULTS[worst])
    assert RESULTS[worst]["ratio_to_bound"] <= 1.0
