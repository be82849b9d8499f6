"""Worker of tests/test_shard_two_sided.py: one process per rank over gloo, NO GPU.  The handle is the stub of
tests/comm_fallback_worker.py built from the device-free cut; shard.ShardComm falls back to torch.distributed and must
move BOTH directions of the halo and of its transpose (the fold).  Evaluation by the CPU oracle."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np
import torch
import torch.distributed as dist

import cases_two_sided as C2
from comm_fallback_worker import StubHandle
from infiniteexamodels.jl_amd import lib as iemlib, shard
from pyoracle import OracleModel


def main():
    name, group = sys.argv[1], int(sys.argv[2])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    gblob = C2.build_core(name).to_blob()
    cut = iemlib.shard_blob(gblob, group, rank, world)
    comm = shard.ShardComm(StubHandle(cut, fail_export=False), dist, force_fallback=True)
    assert comm.kind == "rccl"
    G, L = OracleModel(gblob), OracleModel(cut[0])
    lay = shard.ShardLayout.of_cut(cut)
    xg, yg = C2.eval_point(G)
    xl = xg[lay.var_map].copy()
    xl[lay.halo] = np.nan                       # neither neighbour's values are here yet
    x = torch.from_numpy(xl)
    comm.halo_exchange(x)
    assert np.array_equal(x.numpy(), xg[lay.var_map]), "halo entries (front and back) did not arrive"
    own = lay.owned & ~lay.replicated
    for what, local, ref in (("grad", L.grad(x.numpy()), G.grad(xg)), ("jtprod", L.jtprod(x.numpy(), yg[lay.row_map]), G.jtprod(xg, yg))):
        v = torch.from_numpy(np.ascontiguousarray(local))
        comm.halo_fold(v)
        comm.allreduce_obj_grad(None, v)
        assert not v.numpy()[lay.halo].any(), "halo copies are zeroed by the fold"
        sel = own | lay.replicated
        np.testing.assert_allclose(v.numpy()[sel], ref[lay.var_map][sel], rtol=1e-13, atol=1e-13, err_msg=what)
    dist.barrier()
    if rank == 0:
        print("OK", name, world)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
