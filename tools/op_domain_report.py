#!/usr/bin/env python3
"""Worst relative error per operator and output of the operator-domain sweep (tests/cases_op_domain.py) against the 50-digit
mpmath reference (tests/op_domain_reference.py), for the CPU oracle, the emulated kernels and — where a GPU is visible — the
device:

    python tools/op_domain_report.py [--out profiles/op_domain_errors.json] [--markdown]

cons is the value f, jac_coord / grad carry f', hess_coord carries f''; the products are relative to Σ|addend|.  A backend that
cannot run here (no GPU) is recorded as "not measured".  Imports the tests' helpers; touches no hot path."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODELS = ("unary_sweep", "binary_sweep")
COLUMNS = (("f", ("cons",)), ("f'", ("jac_coord", "grad")), ("f''", ("hess_coord",)))


def measure():
    from infiniteexamodels.jl_amd import lib as iemlib
    import pyoracle
    iemlib.build_library()
    pyoracle.build()
    import op_domain_reference as R
    from emu import EmulatedModel
    gpu = False
    try:
        import torch
        gpu = torch.cuda.is_available()
    except ImportError:
        pass
    res = {"reference": f"sympy derivatives, mpmath at {R.DPS} digits, binary64 inputs taken exactly", "unit": "worst relative error",
           "backends": ["oracle", "emulator", "gpu"], "models": {}}
    for model in MODELS:
        c = R.sweep_case(model)
        evs = {"oracle": c.oe, "emulator": R.EmuEval(c.oe.om, EmulatedModel(c.core, c.blob))}
        gm = None
        if gpu:
            from infiniteexamodels.jl_amd.model import ExaModel
            from test_gpu_op_domain import GpuEval
            gm = ExaModel(c.core, device=0, blob=c.blob)
            evs["gpu"] = GpuEval(c.oe.om, gm, torch)
        table = {}
        for name in res["backends"]:
            if name not in evs:
                continue
            out = c.out_oracle if name == "oracle" else R.outputs(evs[name], c.ref, c.x, c.y, c.v, c.vc)
            for op, d in R.worst_by_owner(model, c.ref, out).items():
                table.setdefault(op, {})[name] = d
        for op in table:
            for name in res["backends"]:
                table[op].setdefault(name, "not measured")
        res["models"][model] = table
        if gm is not None:
            gm.close()
    return res


def markdown(res):
    lines = ["| operator | " + " | ".join(f"{b} {c}" for b in res["backends"] for c, _ in COLUMNS) + " |",
             "|---|" + "---|" * (3 * len(res["backends"]))]
    for model in MODELS:
        for op, row in res["models"][model].items():
            if op in ("obj", "b"):      # the objective's sum and the shared slab: not operators (they are in the JSON)
                continue
            cells = []
            for b in res["backends"]:
                for _, outs in COLUMNS:
                    d = row[b]
                    cells.append("not measured" if isinstance(d, str) else f"{max(d.get(o, 0.0) for o in outs):.1e}")
            lines.append(f"| `{op}` | " + " | ".join(cells) + " |")
    return "\n".join(lines)


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "op_domain_errors.json")
    if "--from" in argv:      # only print the table of a recorded file
        res = json.load(open(argv[argv.index("--from") + 1]))
    else:
        res = measure()
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(f"wrote {out}")
    if "--markdown" in argv:
        print(markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
