"""The two-way halo exchange on ONE GPU (2-4 processes sharing cuda:0, the pattern of tests/test_gpu_comm.py): models
whose stencils reach to the right of their support (forward / central differences, /root/reference/src/transform.jl:535;
the heat workload, transform.jl:141) sharded through iem_create_sharded.  Halo entries on both sides equal the
neighbours' owned values bit for bit, reassembled cons / jac / hess equal the unsharded GPU model bit for bit, fold +
all-reduce equals the unsharded jtprod! within 1e-10, and iem_comm_status is 0 afterwards.  No test provokes a time-out:
tests/test_gpu_comm.py::test_a_skipped_exchange_surfaces_as_an_error covers the poison path both directions share."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("name,group,world,mode", [
    ("central_1d", 1, 2, "eager"), ("central_1d", 1, 3, "graph"), ("central_1d", 1, 4, "async"), ("central_1d", 1, 2, "async_graph"),
    ("forward_1d", 1, 3, "eager"), ("forward_1d", 1, 2, "async"),
    ("heat_central", 2, 3, "eager"), ("heat_central", 2, 2, "async_graph"), ("heat_central", 1, 2, "eager"), ("heat_central", 1, 3, "async"),
    ("heat_forward", 2, 2, "graph")])
def test_two_way_halo_fold_and_allreduce(name, group, world, mode, built):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "comm_worker_two_sided.py"), name, str(group), mode],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    assert "OK" in outs[0], outs[0][-3000:]
