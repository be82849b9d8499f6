#!/usr/bin/env python3
"""profiles/kkt_forms.json: per chain KKT kernel form (tests/cases_kkt_forms.py) what the compiler reports for its kernels
(cross-compiled for gfx950: scratch bytes per lane, VGPRs, LDS per workgroup), and per case what tests/test_gpu_kkt_forms.py
measured on the MI355X (the `KKT_FORMS_JSON` line of a `pytest -s` log: err_cpu, the device's errors, the bound).

    python tools/kkt_forms_profile.py <pytest log of tests/test_gpu_kkt_forms.py>  >  profiles/kkt_forms.json"""
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases_kkt_forms as kf
from infiniteexamodels.jl_amd import lib as iemlib


def usage(shape):
    src, key = iemlib.kkt_source(*shape)
    with tempfile.TemporaryDirectory() as tmp:
        hip = os.path.join(tmp, "k.hip")
        open(hip, "w").write(src)
        flags = src.split("\n", 1)[0][len("// iem-flags:"):].split()
        p = subprocess.run([os.path.join(iemlib.ROCM, "bin", "hipcc"), "--genco", "--offload-arch=gfx950", *flags, "-Rpass-analysis=kernel-resource-usage",
                            "-o", hip + ".hsaco", hip], capture_output=True, text=True, check=True)
    out, cur = {}, None
    for m in re.finditer(r"Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)| VGPRs: (\d+)|LDS Size \[bytes/block\]: (\d+)", p.stderr):
        if m.group(1):
            cur = out.setdefault(m.group(1), {})
        for g, name in ((2, "scratch_bytes_per_lane"), (3, "vgprs"), (4, "lds_bytes")):
            if m.group(g) is not None:
                cur.setdefault(name, int(m.group(g)))
    return "%016x" % key, {k: v for k, v in out.items() if not k.startswith("kkt_hub")}


def main():
    log = open(sys.argv[1]).read()
    measured = json.loads(re.search(r"KKT_FORMS_JSON (\{.*\})$", log, re.M).group(1))
    assert set(measured) == set(kf.BY_ID), "the log does not hold every case"
    with ThreadPoolExecutor(4) as ex:
        compiled = list(ex.map(usage, kf.SHAPES))
    forms = []
    for f, (key, kernels) in zip(kf.FORMS, compiled):
        nb, ne, nc = f["shape"]
        forms.append(dict(shape=[nb, ne, nc], path=f["path"], defines=f["defs"], key=key, declared_lds_bytes=kf.declared_lds(nb, ne, f["defs"]),
                          kkt_eliminate_scratch_bytes_per_lane=kernels["kkt_eliminate"]["scratch_bytes_per_lane"], kernels=kernels,
                          cases={c.id: measured[c.id] for c in kf.CASES if c.shape == f["shape"]}))
    worst = max(measured, key=lambda k: measured[k]["ratio_to_bound"])
    doc = dict(what="chain KKT kernel forms: tests/test_gpu_kkt_forms.py on one MI355X, kernels cross-compiled for gfx950",
               columns="err_cpu: chain_reference against the refined dense solution; x / xB / Dinv / Z / Gp: the device against the same references, "
                       "max |a - b| / max(1, max |b|); bound = 16 max(err_cpu, n 2^-52)",
               worst_case_against_its_bound=dict(case=worst, **measured[worst]), forms=forms)
    json.dump(doc, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
