"""The table of hand-written code objects whose source depends on no model and no shape (csrc/iem_api.cpp: kFixed) as
iem_fixed_source lists it — what build() loops over.  Needs no device."""
import ctypes as C
import re

import pytest

# the kernels the per-object source tests look for (test_kktprod.py, test_kkt_diag.py, test_kkt_border.py, test_barrier.py)
KERNELS = {
    "kkt_diag": ("kkt_gather_d", "kkt_residual_dm", "kkt_axpy_m"),
    "kkt_border": ("kkt_border_ldl", "kkt_border_solve", "kkt_border_colsum", "kkt_border_inertia"),
    "barrier": ("barrier_start", "barrier_terms", "barrier_step", "barrier_update", "barrier_error", "barrier_merit"),
}


def fnv1a64(text: str) -> int:
    h = 1469598103934665603
    for c in text.encode():
        h = ((h ^ c) * 1099511628211) & (2 ** 64 - 1)
    return h


def test_the_list_is_the_three_named_sources(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    listed = list(iemlib.fixed_sources())
    assert [name for name, _, _ in listed] == list(KERNELS)
    named = dict(kkt_diag=iemlib.kkt_diag_source, kkt_border=iemlib.kkt_border_source, barrier=iemlib.barrier_source)
    for name, src, key in listed:
        assert (src, key) == named[name](), name
        assert key == fnv1a64(src), name
        for kernel in KERNELS[name]:
            assert re.search(r"__global__ [^\n]*void " + kernel + r"\(", src), (name, kernel)
    assert len({key for _, _, key in listed}) == len(listed)
    # the key is the hash iem_kkt_source reports for its own text
    src, key = iemlib.kkt_source(40, 0, 12)
    assert key == fnv1a64(src)


@pytest.mark.parametrize("index", [-1, 3])
def test_past_the_end_is_refused_and_writes_nothing(index, built):
    from infiniteexamodels.jl_amd import lib as iemlib
    L = iemlib.lib()
    name, src, key = C.c_char_p(b"untouched"), C.c_void_p(0x5a5a), C.c_uint64(77)
    assert L.iem_fixed_source(index, C.byref(name), C.byref(src), C.byref(key)) == iemlib.IEM_E_ARG == -4
    assert (name.value, src.value, key.value) == (b"untouched", 0x5a5a, 77)
    assert b"iem_fixed_source" in L.iem_last_error()


def test_every_output_is_optional(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    L = iemlib.lib()
    for i, want in enumerate(iemlib.fixed_sources()):
        assert L.iem_fixed_source(i, None, None, None) == 0
        key = C.c_uint64()
        assert L.iem_fixed_source(i, None, None, C.byref(key)) == 0 and key.value == want[2]


def test_precompile_source_wants_the_flag_line(built, tmp_path, monkeypatch):
    from infiniteexamodels.jl_amd import lib as iemlib
    monkeypatch.setattr(iemlib, "KERNEL_DIR", str(tmp_path / "kernels"))
    with pytest.raises(AssertionError):
        iemlib.precompile_source("#include <hip/hip_runtime.h>\n", 1, defer=[])
    assert not (tmp_path / "kernels").exists()      # refused before anything is written
    # a source with the line is taken: its hipcc command carries the line's flags
    jobs = []
    src, key = iemlib.kkt_diag_source()
    out = iemlib.precompile_source(src, key, defer=jobs)
    assert out == str(tmp_path / "kernels" / f"iem_{key:016x}.hsaco") and len(jobs) == 1
    assert "-ffp-contract=off" in jobs[0][0] and "--offload-arch=gfx950" in jobs[0][0]
