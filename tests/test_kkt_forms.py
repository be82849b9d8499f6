"""The chain KKT kernel forms of tests/cases_kkt_forms.py, on the CPU: the generator's data is fit for its purpose, every form
is still the witness of its code path, build() precompiles its code object, and the admission check (kkt_fits, csrc/iem_api.cpp)
is the LDS the kernels declare."""
import ast
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases_kkt_forms as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -4


def test_the_list_is_the_fifteen_forms_and_their_variants():
    assert len(kf.FORMS) == 15 and len(set(kf.SHAPES)) == 15
    ids = [c.id for c in kf.CASES]
    assert len(set(ids)) == len(ids) == 15 * 4 + 6 + 2 + 3 + 3
    assert max(c.n for c in kf.CASES) == 67 * 36 == 2412
    for f in kf.FORMS:      # S = 131: more than 64 survivors and 65 eliminated blocks at level 1; 67: 33 eliminated blocks
        assert f.get("extra_S") == (None if f["defs"]["rowwise"] == 0 else 131 if f["shape"][0] <= 12 else 67)


@pytest.mark.parametrize("case_id", [c.id for c in kf.CASES])
def test_generator_and_restatement_against_the_dense_reference(case_id):
    """(a) chain_reference.factor / solve agree with the refined dense solution, (b) every pivot of the restatement's eliminations
    is at least 1e-3 in size and err_cpu at most 1e-11 — conditions on the GENERATOR —, (c) the negative pivots are the negative
    eigenvalues of the chain part."""
    c, d, r = kf.BY_ID[case_id], kf.data(case_id), kf.reference(case_id)
    nb, ne, nc = c.shape
    assert d.R.size < nc and d.C.size < nc and (d.rows >= 0).sum() == d.R.size and (d.cols >= 0).sum() == d.C.size      # the padding is exercised
    assert (np.intersect1d(d.R, d.C).size == 1) == (c.kind == "shared")
    print(f"{case_id}: n {c.n} err_cpu {r.err_cpu:.3e} (all columns {max(r.err_cols):.3e}) err_inv {r.err_inv:.3e} min |pivot| {r.min_pivot:.3e} "
          f"bound {r.bound:.3e} negative {r.neg}")
    res = np.abs(r.K @ r.x_ref[0] - np.concatenate([d.rhs[0].ravel(), d.rB[0]])).max()
    assert res <= 1e-12 * max(1.0, np.abs(r.x_ref[0]).max())                    # (x_ref does solve the system)
    assert r.min_pivot >= 1e-3
    assert max(r.err_cols) <= 1e-11
    ev = np.linalg.eigvalsh(r.K[:c.S * nb, :c.S * nb])
    assert r.neg == int((ev < 0).sum()) and np.abs(ev).min() > 1e-6
    assert r.neg == c.S * (nb - (nb * 5) // 9)                                   # ... which is the number of constraint rows: K is quasi-definite


def _defines(src):
    head = src.split("#ifndef IEM_KKT_DEVICE_H", 1)[0]
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (KKT_\w+) (-?\d+)$", head, re.M)}


@pytest.mark.parametrize("form", kf.FORMS, ids=lambda f: "%d-%d-%d" % f["shape"])
def test_every_form_is_still_the_witness_of_its_path(form, built):
    """The #define lines at the head of kkt_source(nb, ne, nc) take the values the row's description implies: a retuned kkt_rowwise /
    kkt_shape / kkt_many_width that moves a form to another code path fails here, not silently."""
    from infiniteexamodels.jl_amd import lib as iemlib
    nb, ne, nc = form["shape"]
    src, _ = iemlib.kkt_source(nb, ne, nc)
    got, want = _defines(src), form["defs"]
    assert (got["KKT_NB"], got["KKT_NE"], got["KKT_NC"]) == (nb, ne, nc)
    assert got.get("KKT_ROWWISE", 0) == want["rowwise"] and got.get("KKT_ROW_WPG", 0) == want["wpg"], got
    assert got.get("KKT_WMAX", 4) == want["wmax"] and got.get("KKT_WPE", 0) == want["wpe"] and got["KKT_MR"] == want["mr"], got
    assert iemlib.kkt_many_width(nb, ne, nc) == want["mr"]
    if want["rowwise"]:      # the lanes of the lane-per-row eliminate, as the header derives them: blocks per workgroup, idle lanes
        assert ne == 0
        lpb, lanes = nb // want["rowwise"], 64 * want["wpg"]
        assert (lanes // lpb, lanes % lpb) == form["lanes"]
        assert form["lane_solves"] == (nb <= 32)      # kkt_fz / kkt_fs / kkt_bw up to 32 (kkt_module: lane_rows), the 64-thread solves beyond
    else:                    # the tiles of the panel form: tile rows R, waves W, a partial last tile row per wave, a padded rim
        R = (nb + 15) // 16
        W = min(R, want["wmax"])
        trw = (R + W - 1) // W
        assert (R, W, trw * W > R, not (nb % 16 == 0 and ne % 16 == 0)) == form["tiles"]
    assert (64 if nc <= 8 else 128 if nc <= 16 else 256) == form["update_threads"]      # KKT_TU


def test_build_precompiles_every_form(built):
    """No test compiles a chain code object: build() reads the same list, and the 15 code objects are in the in-tree cache."""
    from infiniteexamodels.jl_amd import lib as iemlib
    tree = ast.parse(open(os.path.join(ROOT, "__graft_entry__.py")).read())
    loops = [n for n in ast.walk(tree) if isinstance(n, ast.For) and ast.unparse(n.iter) == "cases_kkt_forms.SHAPES"]
    assert len(loops) == 1 and "precompile_source" in ast.unparse(loops[0]) and "kkt_source(*shape)" in ast.unparse(loops[0])
    keys = {shape: iemlib.kkt_source(*shape)[1] for shape in kf.SHAPES}
    assert len(set(keys.values())) == 15
    for shape, key in keys.items():
        assert os.path.exists(os.path.join(iemlib.KERNEL_DIR, "iem_%016x.hsaco" % key)), ("build() precompiles the code object of", shape)


# ---- admission: kkt_fits is the LDS the kernels declare -------------------------------------------------------------------------
def _admitted(L, nb, ne, nc):
    p, key = C.c_void_p(), C.c_uint64()
    rc = L.iem_kkt_source(nb, ne, nc, C.byref(p), C.byref(key))
    if rc == 0:
        L.iem_free(p)
    else:
        assert rc == E_ARG and b"within the LDS of a CU" in L.iem_last_error()
    return rc == 0


def test_admission_is_the_declared_lds(built):
    """Over all nb and ne in steps of 4 (and ne = -1): iem_kkt_source admits a shape if and only if the LDS kkt_eliminate declares for it
    (cases_kkt_forms.declared_lds, restated from the header) is within 163 840 bytes.  (kkt_module judges a shape by the same kkt_admit: tests/test_gpu_kkt_forms.py
    asks the chain calls themselves, on a real handle.)"""
    from infiniteexamodels.jl_amd import lib as iemlib
    L = iemlib.lib()
    largest = {}
    for nb in range(4, 100, 4):
        for ne in [-1] + list(range(0, 132, 4)):
            want = kf.declared_lds(nb, ne) <= kf.LDS_BYTES
            assert _admitted(L, nb, ne, 4) == want, (nb, ne, kf.declared_lds(nb, ne))
            if want:
                largest[nb] = ne
    assert all(largest[nb] == 128 for nb in range(4, 64, 4)) and largest[84] == 64 and largest[68] == 100 and largest[96] == NE_MAX_96
    assert kf.declared_lds(84, 64) == 158888 and kf.declared_lds(84, 68) == 164264 and kf.declared_lds(68, 104) == 163880
    # the two shapes the old rule (panels sized from nb) let through to a compiler error
    assert not _admitted(L, 84, 68, 4) and not _admitted(L, 68, 104, 4)
    # kkt_update's side, unchanged: 56 nc (nc + 1) + 1024 at the largest nc
    assert _admitted(L, 48, 0, 48) and 56 * 48 * 49 + 1024 <= kf.LDS_BYTES
    # the other limits, one each: one rule for the source and for the module
    for shape in ((0, 0, 4), (100, 0, 4), (22, 0, 4), (20, 6, 4), (20, 132, 4), (20, -2, 4), (20, 0, 0), (20, 4, 0), (20, 0, 6), (20, 0, 52), (8, 0, 12)):
        assert not _admitted(L, *shape), shape


NE_MAX_96 = 44
BOUNDARY = [(84, 64, 4), (68, 100, 4), (96, NE_MAX_96, 4)]
LANE_PER_ROW = [(12, 0, 4), (36, 0, 12)]      # the other branch of the formula: rows per lane 2 and 1, both with a two-wave workgroup


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("shape", BOUNDARY + LANE_PER_ROW, ids=lambda s: "%d-%d-%d" % s)
def test_the_boundary_shapes_compile_at_the_restated_lds(shape, tmp_path, built):
    """The largest admitted border at nb = 84, 68 and 96, and two lane-per-row shapes: the compiler's own resource-usage remark for
    kkt_eliminate is the restated number."""
    from infiniteexamodels.jl_amd import lib as iemlib
    nb, ne, nc = shape
    if shape in BOUNDARY:
        assert kf.declared_lds(nb, ne) <= kf.LDS_BYTES < kf.declared_lds(nb, ne + 4)
    else:
        assert kf.declared_lds(nb, ne) == {12: 4040, 36: 1736}[nb]
    src, _ = iemlib.kkt_source(*shape)
    hip = tmp_path / "k.hip"
    hip.write_text(src)
    flags = src.split("\n", 1)[0][len("// iem-flags:"):].split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", *flags, "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(hip) + ".hsaco", str(hip)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lds, cur = {}, None
    for m in re.finditer(r"Function Name: (\S+)|LDS Size \[bytes/block\]: (\d+)", p.stderr):
        if m.group(1):
            cur = m.group(1)
        else:
            lds[cur] = int(m.group(2))
    print(shape, lds["kkt_eliminate"], lds["kkt_update"])
    assert lds["kkt_eliminate"] == kf.declared_lds(nb, ne)
    assert lds["kkt_update"] <= 56 * nc * (nc + 1) + 1024
