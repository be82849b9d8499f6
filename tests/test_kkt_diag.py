"""A per-row diagonal in the constraint block of the C-ABI's KKT object (iem_kkt_assemble_diag / iem_kkt_residual_diag /
iem_kkt_solve_refined_diag, csrc/iem_kkt_diag_device.h) — what needs no device: the gather plan and the block cyclic reduction
with sixteen decades of dcon (numpy restatements), the new code object's source, the keys of the other KKT code objects, the
Python operator with a tensor delta_c, and the argument checks."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import chain_reference as ref
import kkt_diag_reference as dref
from kkt_diag_reference import DC, DW

MODELS = ["quadrotor_5", "quadrotor_100", "opf_7", "farmer_5", "pandemic_20x3", "pandemic_100x7"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kkt_source_keys.json")
_HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("name", MODELS)
def test_plan_and_numerics_with_a_per_row_diagonal(name, built):
    """The plan of iem_kkt_analyse_blob over the virtual source array whose row segment is −(dcon + delta_c) fills the blocks of
    scipy's [[H + diag(sigma + delta_w), J'], [J, −diag(dcon + delta_c)]]; the block cyclic reduction on them, one step of refinement:
    the residual meets the criterion of tests/test_kkt_cabi.py, and the pivot signs are the inertia of K.  (Passes without the
    feature: the plan and the factorisation need no change for dcon in 0 | 1e-8 .. 1e8.)"""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.kkt_chain import ChainLayout
    s = dref.host_system(name)
    om, K, rhs = s["om"], s["K"], s["rhs"]
    n = om.nvar + om.ncon
    jr, jc = om.jac_structure()
    L = ChainLayout(s["core"].slabs, om.nvar, om.ncon, jr, jc)
    info, blk, loc, rows, cols, dest, seg, perm = iemlib.kkt_analyse_blob(s["blob"])
    src = dref.gather_sources(om.hess_coord(s["x"], s["y"], 1.0), om.jac_coord(s["x"]), s["sigma"], s["dcon"], DW, DC, om.nvar, om.ncon)
    assert np.array_equal(src[-1 - om.ncon:-1], -(s["dcon"] + DC))
    flat = dref.gather(info["block_doubles"], dest, seg, perm, src)
    D, B, E, G = ref.fill_blocks(L, np.repeat(np.arange(n), np.diff(K.indptr)), K.indices, K.data)
    oD, oB, oE, oG, total = L.offsets()
    assert total == info["block_doubles"]
    # an entry is a sum of at most `terms` sources in another order than scipy's: terms·2⁻⁵² relative to the largest value summed —
    # the COO values for the sums, the entry itself where one large diagonal term (dcon up to 1e8) stands alone
    terms = int(np.diff(seg.astype(np.int64)).max())
    big = max(1.0, np.abs(src[:-1 - om.ncon - om.nvar]).max())
    close = lambda a, b: np.allclose(a, b, rtol=terms * 2.0 ** -52, atol=terms * 2.0 ** -52 * big)
    assert close(flat[oD:oB].reshape(L.S, L.nb, L.nb), D)
    if L.reach > 0:
        assert close(flat[oB:oE].reshape(L.S, L.nc, L.nc)[:, :L.rowsR.size, :L.colsC.size], B[:, L.rowsR[:, None], L.colsC[None, :]])
    assert close(flat[oE:oG].reshape(L.S, L.nb, L.ne), E) and close(flat[oG:total].reshape(L.ne, L.ne), G)
    # factor / solve on the blocks the plan filled
    Dg, Eg, Gg = flat[oD:oB].reshape(L.S, L.nb, L.nb), flat[oE:oG].reshape(L.S, L.nb, L.ne), flat[oG:total].reshape(L.ne, L.ne)
    Dinv, X, Y, Z, Gp, neg = ref.factor(Dg, B, Eg)
    on, pos, border = L.positions()

    def solve(b):
        r = np.zeros(L.S * L.nb); r[pos] = b[on]
        rB = np.zeros(L.ne); rB[:L.n_border] = b[border]
        xs, xB = ref.solve(Dinv, X, Y, Z, Gg, Gp, r.reshape(L.S, L.nb), rB)
        out = np.empty(n); out[on] = xs.reshape(-1)[pos]; out[border] = xB[:L.n_border]
        return out
    sol = solve(rhs)
    sol = sol + solve(rhs - K @ sol)
    ok, resid, comp = dref.residual_ok(K, sol, rhs)
    print(name, "n", n, "residual after one step", resid, "componentwise", comp)
    assert ok
    if s["neg"] is not None:
        neg += int((np.linalg.eigvalsh(Gg - Gp.sum(0)) < 0).sum()) if L.ne else 0
        assert neg == s["neg"] and neg >= om.ncon


def test_the_new_source(built, tmp_path):
    """a code object of its own, compiled without contraction: the three kernels, the integer maximum as its only atomic, no scratch"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.kkt_diag_source()
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    for kernel in ("kkt_gather_d", "kkt_residual_dm", "kkt_axpy_m"):
        assert re.search(r"__global__ [^\n]*void " + kernel + r"\(", src), kernel
    assert "atomicMax(" in src and "atomicAdd" not in src and len(re.findall(r"\batomic\w+\(", src)) == 1
    assert key != iemlib.kkt_border_source()[1]
    if not os.path.exists(_HIPCC):
        pytest.skip("no hipcc")
    hip = tmp_path / "d.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "d.hsaco"), str(hip)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "d.hsaco").stat().st_size > 1000
    usage, cur = {}, None
    for m in re.finditer(r"Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)", p.stderr):
        if m.group(1):
            cur = m.group(1)
        else:
            usage[cur] = int(m.group(2))
    assert usage == {"kkt_gather_d": 0, "kkt_residual_dm": 0, "kkt_axpy_m": 0}, usage


def test_keys_of_the_other_kkt_code_objects_did_not_move(built):
    """every KKT code object and the barrier object keep the key pinned in tests/golden/kkt_source_keys.json"""
    from infiniteexamodels.jl_amd import lib as iemlib
    want = json.load(open(GOLDEN))
    # (20,0,4 — the hub lanes' chains — stood here as "20,4,0": nb 20, ne 4, nc 0, a shape no handle loads; iem_kkt_source refuses it now)
    assert set(want["iem_kkt_source"]) == {"40,0,12", "20,0,8", "20,112,4", "20,0,4", "96,-1,4"}
    with pytest.raises(iemlib.IemError):
        iemlib.kkt_source(20, 4, 0)
    for shape, key in want["iem_kkt_source"].items():
        assert f"{iemlib.kkt_source(*map(int, shape.split(',')))[1]:016x}" == key, shape
    assert set(want) == {"iem_kkt_source", "iem_kkt_border_source", "iem_kkt_diag_source", "iem_barrier_source"}
    assert f"{iemlib.kkt_border_source()[1]:016x}" == want["iem_kkt_border_source"]
    assert f"{iemlib.kkt_diag_source()[1]:016x}" == want["iem_kkt_diag_source"]
    assert f"{iemlib.barrier_source()[1]:016x}" == want["iem_barrier_source"]


def test_matrix_free_kkt_with_a_tensor_delta_c(built):
    """MatrixFreeKKT with delta_c a tensor of ncon entries against scipy (the host stand-in and the 1e-10 relative of
    tests/test_kktprod.py); a float delta_c keeps the bits of the expression it had."""
    import torch
    from host_model import HostModel
    from infiniteexamodels.jl_amd.kkt_chain import MatrixFreeKKT
    from test_kktprod import TOL, bits, point, rel, setup

    for name in ("quadrotor_5", "pandemic_20x3", "farmer_5"):
        core, blob, om, em, own = setup(name)

        class Host(HostModel):
            def kktprod(self, x, y, u, v=None, obj_weight=1.0, out_x=None, out_y=None):
                ox, oy = em.kktprod(self._np(x), self._np(y), self._np(u), None if v is None else self._np(v), float(obj_weight))
                out_x.copy_(torch.from_numpy(ox.copy())); out_y.copy_(torch.from_numpy(oy.copy()))
                return out_x, out_y
        hm = Host(blob)
        x, y, _, _ = point(name, om)
        n, mc = om.nvar, om.ncon
        sigma, dcon, _ = dref.diag_inputs(n, mc)
        rng = np.random.default_rng(9)
        z, rhs = rng.standard_normal(n + mc), rng.standard_normal(n + mc)
        K = dref.host_kkt_diag(om, x, y, sigma, 1e-3, dcon + 1e-4, 0.7)
        tx, ty, ts, tz = (torch.from_numpy(a) for a in (x, y, sigma, z))
        op = MatrixFreeKKT(hm, tx, ty, 0.7, ts, 1e-3, torch.from_numpy(dcon + 1e-4))
        assert rel(op.matvec(tz).numpy(), K @ z) <= TOL
        assert rel(op.residual(torch.from_numpy(rhs), tz).numpy(), rhs - K @ z) <= TOL
        with pytest.raises(ValueError):
            MatrixFreeKKT(hm, tx, ty, 0.7, ts, 1e-3, torch.zeros(mc + 1, dtype=torch.float64))
        # a float: out_y − delta_c·z_y on kktprod's output, rounded as before
        opf = MatrixFreeKKT(hm, tx, ty, 0.7, ts, 1e-3, 1e-4)
        ox, oy = em.kktprod(x, y, z[:n], z[n:], 0.7)
        want = np.concatenate([ox + (sigma + 1e-3) * z[:n], oy - 1e-4 * z[n:]])
        assert isinstance(opf.delta_c, float) and np.array_equal(bits(opf.matvec(tz).numpy()), bits(want))


def test_argument_checks_that_need_no_device(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.kkt_chain import KKTObject
    L = iemlib.lib()
    for name in ("iem_kkt_assemble_diag", "iem_kkt_residual_diag", "iem_kkt_solve_refined_diag", "iem_kkt_diag_source"):
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None
    assert len(L.iem_kkt_assemble_diag.argtypes) == 7 and len(L.iem_kkt_residual_diag.argtypes) == 16 and len(L.iem_kkt_solve_refined_diag.argtypes) == 15
    import torch
    obj = KKTObject.__new__(KKTObject)      # (no handle: the check comes before anything touches the library)
    obj._at, obj._torch = None, torch
    with pytest.raises(ValueError, match="at="):
        obj.solve(torch.zeros(4, dtype=torch.float64), refine=1)
    with pytest.raises(ValueError, match="at="):
        obj.residual(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))
    # null / range refusals of the C calls come before any device work
    assert L.iem_kkt_assemble_diag(None, None, None, None, None, 0.0, 0.0) == -4
    assert L.iem_kkt_residual_diag(None, None, None, 1.0, None, None, 0.0, 0.0, 1, None, 0, None, 0, None, 0, None) == -4
    assert L.iem_kkt_solve_refined_diag(None, None, None, 1.0, None, None, 0.0, 0.0, 1, None, 0, None, 0, 1, None) == -4
