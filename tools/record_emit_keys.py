#!/usr/bin/env python3
"""Record what the generator emits for every small test model under a list of option sets:
the key of `lib.emit_source` (FNV of the full source, device header included) and the first 16 hex
digits of the SHA-256 of `lib.emit_launch_plan`'s text (kernels, grids, LDS, tables).

    python tools/record_emit_keys.py            # writes tests/golden/emit_keys_options.json
    python tools/record_emit_keys.py --programs # writes tests/golden/emit_keys_all_programs.json: each of the nine programs
                                                # (selected by its public option) under PROGRAM_OPTION_SETS, source hash included,
                                                # and the error text of every two program options set together

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


GOLDEN_PROGRAMS = os.path.join(ROOT, "tests", "golden", "emit_keys_all_programs.json")

# the nine programs by their public options, in the generator's order
PROGRAMS = [{}, {"param_kinds": 1}, {"param_kinds": 2}, {"param_kinds": 3}, {"param_kinds": 4}, {"param_kinds": 5},
            {"scaled_kinds": 1}, {"kkt_kinds": 1}, {"scaled_phase_kinds": 1}]
PROGRAM_OPTION_SETS = [
    {}, {"carrier": 1}, {"split_small": 0}, {"jac_split": 0}, {"phase_kernels": 0}, {"no_fuse": 1}, {"fuse_groups": 0},
    {"hess_merge": 1}, {"fold_colloc": 0}, {"big_batch_jac": 1, "big_batch_hess": 1}, {"det_scatter": 2}, {"det_scatter": 0},
    {"name_tag": 34},
]
# two program options at once: refused, whichever model
PROGRAM_PAIRS = [{"param_kinds": p, k: 1} for p in (1, 5) for k in ("scaled_kinds", "kkt_kinds", "scaled_phase_kinds")] + [
    {"scaled_kinds": 1, "kkt_kinds": 1}, {"scaled_kinds": 1, "scaled_phase_kinds": 1}, {"kkt_kinds": 1, "scaled_phase_kinds": 1}]
PAIRS_MODEL = "quadrotor_5"


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


def program_model_blobs() -> dict:
    """name -> blob of every model the derived programs are tested on, and those of model_blobs()."""
    import cases_param
    import cases_scaled
    blobs = {n: cases_param.build_core(n).to_blob() for n in cases_param.NAMES + cases_param.NO_PARAM}
    blobs["nan_and_constant_rows"] = cases_scaled.nan_and_constant_rows().to_blob()
    for n, b in model_blobs().items():
        assert blobs.setdefault(n, b) == b, n
    return blobs


def program_records(blob: bytes) -> dict:
    """program -> option set -> "<emit key> <source sha> <plan sha>" (or "error: text") of one blob."""
    out = {}
    for prog in PROGRAMS:
        recs = out[set_name(prog)] = {}
        for opts in PROGRAM_OPTION_SETS:
            r = emit_record(blob, {**opts, **prog}, source_sha=True)
            recs[set_name(opts)] = "error: " + r["error"] if "error" in r else f"{r['emit_key']} {r['source_sha256_16']} {r['plan_sha256_16']}"
    return out


def pair_records(blob: bytes) -> dict:
    return {set_name(pair): emit_record(blob, pair)["error"] for pair in PROGRAM_PAIRS}


def emit_record(blob: bytes, opts: dict, dump: str = None, source_sha: bool = False) -> dict:
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
    if source_sha:
        return {"emit_key": f"{key:016x}", "source_sha256_16": hashlib.sha256(src.encode()).hexdigest()[:16],
                "plan_sha256_16": hashlib.sha256(plan.encode()).hexdigest()[:16]}
    return {"emit_key": f"{key:016x}", "plan_sha256_16": hashlib.sha256(plan.encode()).hexdigest()[:16]}


def dump_programs(out: dict, path: str):
    """The golden file of --programs, compact: per model and program ONE line, each distinct record once with the indices (into
    "option_sets") of the option sets that gave it."""
    names = [set_name(o) for o in PROGRAM_OPTION_SETS]
    with open(path, "w") as f:
        f.write('{"option_sets": ' + json.dumps(names) + ',\n"models": {\n')
        for i, (m, v) in enumerate(sorted(out["models"].items())):
            f.write(f' {json.dumps(m)}: {{"blob_sha256_16": "{v["blob_sha256_16"]}", "programs": {{\n')
            for j, (prog, sets) in enumerate(sorted(v["programs"].items())):
                by_rec = {}
                for s in names:
                    by_rec.setdefault(sets[s], []).append(names.index(s))
                f.write(f'  {json.dumps(prog)}: {json.dumps(by_rec)}' + (",\n" if j + 1 < len(v["programs"]) else "}}"))
            f.write(",\n" if i + 1 < len(out["models"]) else "},\n")
        f.write('"pairs": ' + json.dumps(out["pairs"], indent=0, sort_keys=True) + "}\n")


def load_programs(path: str = GOLDEN_PROGRAMS) -> dict:
    """... and back: {"models": {name: {"blob_sha256_16", "programs": {program: {option set: record}}}}, "pairs": {...}}."""
    raw = json.load(open(path))
    names = raw["option_sets"]
    for v in raw["models"].values():
        v["programs"] = {prog: {names[i]: rec for rec, idx in by_rec.items() for i in idx} for prog, by_rec in v["programs"].items()}
    return {"models": raw["models"], "pairs": raw["pairs"]}


def main_programs(argv):
    blobs = program_model_blobs()
    out = {"models": {n: {"blob_sha256_16": hashlib.sha256(b).hexdigest()[:16], "programs": program_records(b)} for n, b in blobs.items()},
           "pairs": pair_records(blobs[PAIRS_MODEL])}
    n = sum(len(s) for m in out["models"].values() for s in m["programs"].values()) + len(out["pairs"])
    if "--check" in argv:
        want = load_programs()
        bad = [f"{m}: {p}: {s}" for m, v in out["models"].items() for p, sets in v["programs"].items() for s, r in sets.items()
               if want["models"].get(m, {}).get("programs", {}).get(p, {}).get(s) != r]
        bad += [f"pair {p}" for p, e in out["pairs"].items() if want["pairs"].get(p) != e]
        print(f"{n} entries, {len(bad)} differ" + "".join(f"\n  {b}" for b in bad))
        return 1 if bad else 0
    dump_programs(out, GOLDEN_PROGRAMS)
    print(f"wrote {GOLDEN_PROGRAMS}: {len(blobs)} models x {len(PROGRAMS)} programs x {len(PROGRAM_OPTION_SETS)} option sets, {len(PROGRAM_PAIRS)} pairs")
    return 0


def main(argv):
    from infiniteexamodels.jl_amd import lib as iemlib
    iemlib.build_library()
    if "--programs" in argv:
        return main_programs(argv)
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
