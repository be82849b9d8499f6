#!/usr/bin/env python3
"""jac_coord! / hess_coord! of the large 4-group model (tests/cases_many_groups.py: y(t, x, a, b),
100 x 20 x 10 x 10 supports) in three configurations of the same model:

  digits    the box the producer writes (a product of four groups folded into three runs), run digits
            decoded in registers (digit_fields=1, the default)
  gathers   the same blob with the short digit columns read (digit_fields=0)
  explicit  every template as a 1-D explicit list (what a foreign producer writes)

Timed in blocks of back-to-back launches between one event pair, alternating the encodings, three
rounds; the median block is reported.  Bytes are the launch plan's algorithmic traffic (rbytes +
wbytes of the kernels of that kind) and their fraction of 8 TB/s at the measured time.

  python tools/many_groups_bench.py [--reps 50] [--out profiles/many_groups_ab.json]
"""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

import cases_many_groups as MG
from infiniteexamodels.jl_amd import lib as iemlib
from infiniteexamodels.jl_amd.items import Field, Items
from infiniteexamodels.jl_amd.model import ExaModel

KINDS = {"jac": 1, "hess": 2}


def explicit(core):
    c = copy.copy(core)
    tpls = []
    for t in core.templates:
        u = copy.copy(t)
        d = t.items.dims
        u.ifields = [Field("int", "gather", 0, (1,), np.ascontiguousarray(f.values(d), dtype=np.int64)) for f in t.ifields]
        u.ffields = [Field("float", "gather", 0, (1,), np.ascontiguousarray(f.values(d), dtype=np.float64)) for f in t.ffields]
        u.items = Items((len(t.items),), {})
        tpls.append(u)
    c.templates = tpls
    return c.to_blob()


def plan(blob):
    out = {k: {"kernels": 0, "rbytes": 0, "wbytes": 0} for k in KINDS}
    for line in iemlib.emit_launch_plan(blob).splitlines():
        w = line.split()
        if w and w[0] == "kernel":
            for k, kind in KINDS.items():
                if int(w[3]) == kind:
                    out[k]["kernels"] += 1
                    out[k]["rbytes"] += int(w[11])
                    out[k]["wbytes"] += int(w[13])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_groups_ab.json"))
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        core = MG.build_core("large_four_groups")
    folded = core.to_blob()
    blobs = {"digits": folded, "gathers": folded, "explicit": explicit(core)}
    opts = {"digits": {"digit_fields": 1}, "gathers": {"digit_fields": 0}, "explicit": {}}
    models = {k: ExaModel.from_blob(b, device=0, options=opts[k]) for k, b in blobs.items()}
    gm = models["digits"]
    x = np.abs(gm.meta.x0 + 0.1 * np.random.default_rng(0).standard_normal(gm.meta.nvar)) + 0.05
    y = np.random.default_rng(1).standard_normal(gm.meta.ncon)
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    jac = torch.empty(gm.meta.nnzj, dtype=torch.float64, device="cuda")
    hess = torch.empty(gm.meta.nnzh, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(m, kind):
        if kind == "jac":
            return m._L.iem_jac_coord(m._h, ptr(xd), ptr(jac))
        return m._L.iem_hess_coord(m._h, ptr(xd), ptr(yd), C.c_double(1.0), ptr(hess))

    ref = {}
    for name, m in models.items():   # both encodings compute the same bytes
        m.jac_coord(xd, jac)
        m.hess_coord(xd, yd, hess)
        ref[name] = (jac.cpu().numpy().copy(), hess.cpu().numpy().copy())
    same = all(np.array_equal(ref["digits"][i], ref[o][i]) for o in ("gathers", "explicit") for i in (0, 1))

    times = {n: {k: [] for k in KINDS} for n in models}
    for _ in range(3):
        for kind in KINDS:
            for name, m in models.items():
                for _ in range(5):
                    iemlib.check(call(m, kind))
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                for _ in range(a.reps):
                    call(m, kind)
                e.record()
                e.synchronize()
                times[name][kind].append(s.elapsed_time(e) * 1e3 / a.reps)
    res = {"model": "large_four_groups", "items_per_template": int(max(len(t.items) for t in core.templates)),
           "nvar": int(gm.meta.nvar), "ncon": int(gm.meta.ncon), "nnzj": int(gm.meta.nnzj), "nnzh": int(gm.meta.nnzh),
           "reps_per_block": a.reps, "identical_outputs": bool(same), "encodings": {}}
    for name, b in blobs.items():
        with iemlib.options(**opts[name]):
            pl = plan(b)
        res["encodings"][name] = {}
        for kind in KINDS:
            us = float(np.median(times[name][kind]))
            byt = pl[kind]["rbytes"] + pl[kind]["wbytes"]
            res["encodings"][name][kind] = {"us": round(us, 2), "blocks_us": [round(v, 2) for v in times[name][kind]],
                                            "kernels_per_call": pl[kind]["kernels"], "rbytes": pl[kind]["rbytes"],
                                            "wbytes": pl[kind]["wbytes"], "frac_of_8TBps": round(byt / (us * 1e-6) / 8e12, 3)}
    txt = json.dumps(res, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()
