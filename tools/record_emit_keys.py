#!/usr/bin/env python3
"""Record what the generator emits for every small test model under a list of option sets:
the key of `lib.emit_source` (FNV of the full source, device header included) and the first 16 hex
digits of the SHA-256 of `lib.emit_launch_plan`'s text (kernels, grids, LDS, tables).

    python tools/record_emit_keys.py            # writes tests/golden/emit_keys_options.json

A refactor of csrc/iem_codegen.cpp that must not change the generated code runs this on its PARENT
commit and commits the file; tests/test_many_groups.py::test_emit_keys_under_options then holds the
refactored generator to it.  An option set a model refuses is recorded as its error text.  CPU only."""
import hashlib
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "emit_keys_options.json")

# each on top of the defaults
OPTION_SETS = [
    {}, {"carrier": 1}, {"split_small": 0}, {"jac_split": 0}, {"carrier": 1, "split_small": 0}, {"pair_kernel": 0},
    {"phase_kernels": 0}, {"no_fuse": 1}, {"fuse_groups": 0}, {"no_fuse": 1, "fuse_groups": 2}, {"hess_merge": 1},
    {"store_mode": 0}, {"store_mode": 1}, {"flat2d": 1}, {"xcd_remap": 1}, {"fold_colloc": 0}, {"fold_colloc": 1},
    {"name_tag": 34},
    {"big_batch_jac": 1, "big_batch_hess": 1},   # the large-grid shape, two tile sizes in one program
    {"big_batch_jac": 1},                        # jac and hess at different tiles: no pair, no accepted phase
    {"obj_wgs": 4},
]


def set_name(opts: dict) -> str:
    return " + ".join(f"{k}={v}" for k, v in opts.items()) or "defaults"


def model_blobs() -> dict:
    """name -> blob of every model of tests/cases.py::small_cases() and tests/cases_many_groups.py::many_group_cases()."""
    import cases
    import cases_many_groups as MG
    from infiniteexamodels.jl_amd import transcribe
    blobs = {n: cases.build_core(n).to_blob() for n in cases.small_cases()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n, make in MG.many_group_cases().items():
            blobs[n] = transcribe.exa_core(make(), transcribe.ExaMappingData()).to_blob()
    return blobs


def emit_record(blob: bytes, opts: dict, dump: str = None) -> dict:
    """{"emit_key", "plan_sha256_16"} of one blob under one option set, or {"error": text}."""
    from infiniteexamodels.jl_amd import lib as iemlib
    try:
        with iemlib.options(**opts):
            src, key = iemlib.emit_source(blob)
            plan = iemlib.emit_launch_plan(blob)
    except iemlib.IemError as e:
        return {"error": str(e)}
    if dump:
        with open(dump + ".hip", "w") as f:
            f.write(src)
        with open(dump + ".plan", "w") as f:
            f.write(plan)
    return {"emit_key": f"{key:016x}", "plan_sha256_16": hashlib.sha256(plan.encode()).hexdigest()[:16]}


def main(argv):
    from infiniteexamodels.jl_amd import lib as iemlib
    iemlib.build_library()
    dump = argv[argv.index("--dump") + 1] if "--dump" in argv else None   # full texts, for diffing two generators
    if dump:
        os.makedirs(dump, exist_ok=True)
    out = {}
    for name, blob in model_blobs().items():
        out[name] = {"blob_sha256_16": hashlib.sha256(blob).hexdigest()[:16], "sets": {}}
        for opts in OPTION_SETS:
            s = set_name(opts)
            out[name]["sets"][s] = emit_record(blob, opts, dump and os.path.join(dump, f"{name}__{s.replace(' ', '')}"))
    if "--check" in argv:
        want = json.load(open(GOLDEN))
        bad = [(n, s) for n in out for s in out[n]["sets"] if want.get(n, {}).get("sets", {}).get(s) != out[n]["sets"][s]]
        print(f"{sum(len(v['sets']) for v in out.values())} entries, {len(bad)} differ" + "".join(f"\n  {n}: {s}" for n, s in bad))
        return 1 if bad else 0
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(out)} models x {len(OPTION_SETS)} option sets")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
