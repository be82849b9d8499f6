"""The generator's program table (csrc/iem_codegen.cpp: kPrograms) against the generator BEFORE it had one: emit key, source
hash and launch-plan hash of each of the nine programs, selected by its public option, of every test model under the option
sets of tools/record_emit_keys.py --programs, and the refusal of every two program options set together
(tests/golden/emit_keys_all_programs.json, recorded at the parent of the commit that introduced the table).  CPU only."""
import functools
import hashlib
import os
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import record_emit_keys as rk  # noqa: E402

WANT = rk.load_programs()


@functools.lru_cache(maxsize=None)
def _blobs():
    return rk.program_model_blobs()


@pytest.mark.parametrize("name", sorted(WANT["models"]))
def test_every_program_is_byte_identical(name, built):
    want = WANT["models"][name]
    blob = _blobs()[name]
    assert hashlib.sha256(blob).hexdigest()[:16] == want["blob_sha256_16"]
    got = rk.program_records(blob)
    assert list(got) == [rk.set_name(p) for p in rk.PROGRAMS] and sorted(got) == sorted(want["programs"])
    for prog, sets in got.items():
        assert sorted(sets) == sorted(want["programs"][prog]) and len(sets) == len(rk.PROGRAM_OPTION_SETS) == 13
        for s, rec in sets.items():
            assert rec == want["programs"][prog][s], (name, prog, s)


def test_models_and_refused_pairs(built):
    """The golden file holds every model the tool lists; two program options at once are refused with the recorded text."""
    assert sorted(_blobs()) == sorted(WANT["models"])
    got = rk.pair_records(_blobs()[rk.PAIRS_MODEL])
    assert len(got) == 9 and got == WANT["pairs"]
    for pair, text in got.items():
        first, second = text.split(": ", 1)[1].split(" and ", 1)
        assert {first, second.split()[0]} == {o.split("=")[0] for o in pair.split(" + ")}, (pair, text)
