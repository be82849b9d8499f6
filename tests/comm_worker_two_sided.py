"""Worker of tests/test_gpu_comm_two_sided.py: one process per rank, all ranks on cuda:0, like tests/comm_worker.py — for
models whose stencils reach to the right of their support (forward / central differences,
/root/reference/src/transform.jl:535).  Each rank holds only its owned slice of a DISTRIBUTED x: the halo entries on BOTH
sides arrive through one iem_halo_exchange (stand-alone, or riding on an evaluation launch), J'v folds back both ways
(iem_halo_fold), the replicated entries are summed by iem_allreduce_obj_grad.  gloo only moves the mailbox handles and
gathers the results for checking."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np
import torch
import torch.distributed as dist

import cases_two_sided as C2
from infiniteexamodels.jl_amd import shard, transcribe
from infiniteexamodels.jl_amd.model import ExaModel

SIZES = C2.COMM_MODELS


def _same_bits(got, ref, what):
    bad = np.nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} entries differ, first at {bad[:8].tolist()}: got {got[bad[:4]].tolist()} ref {ref[bad[:4]].tolist()}"


def main():
    name, group, mode = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    use_graph, use_async = mode in ("graph", "async_graph"), mode in ("async", "async_graph")
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    opts = {"split_small": 0}
    gcore = transcribe.exa_core(SIZES[name]())
    gblob = gcore.to_blob()
    gm = ExaModel.sharded(gblob, group, rank, world, device=0, options=opts)
    info, halo2 = gm.shard_info(), gm.shard_halo()
    along_t = name.startswith("heat") and group == 1
    want = (1, 0) if along_t else {"central_1d": (1, 1), "forward_1d": (0, 1), "heat_central": (1, 1), "heat_forward": (0, 1)}[name]
    assert (halo2["reach_left"], halo2["reach_right"]) == want, halo2
    assert halo2["halo_left"] == (want[0] if rank else 0) and halo2["halo_right"] == (want[1] if rank + 1 < world else 0), halo2
    shard.connect_mailboxes(gm, dist)
    lay = shard.ShardLayout.of_model(gm)
    vm, halo, repl, owned = lay.var_map, lay.halo, lay.replicated, lay.owned
    row_map, jpos, hpos = lay.row_map, lay.jac_pos, lay.hess_pos
    assert int(lay.halo_right.sum()) * max(want[1], 1) == halo2["doubles_to_left"] * halo2["halo_right"]
    if rank == 0:
        from pyoracle import OracleModel
        G = ExaModel(gcore, device=0, blob=gblob, options=opts)
        O = OracleModel(gblob)
    nvg, ncg = info["nvar_global"], info["ncon_global"]
    new = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")
    xd, yd, g, c, jv, hv, jt = new(gm.meta.nvar), new(gm.meta.ncon), new(gm.meta.nvar), new(gm.meta.ncon), new(gm.meta.nnzj), new(gm.meta.nnzh), new(gm.meta.nvar)
    f = torch.zeros(1, dtype=torch.float64, device="cuda")
    exchange = gm.halo_exchange_async if use_async else gm.halo_exchange
    reads = gm.halo_reads()
    if lay.halo.any():   # linear difference rows: cons! reads the neighbours on both sides, the partials are item data
        assert reads["cons"][0] and not reads["cons"][2] and not reads["jac"][0] and not reads["hess"][0], reads
        if name.endswith("_1d"):
            assert reads["jac"][2] and reads["hess"][2], reads          # ... so they may carry the two-way exchange

    def loop():
        exchange(xd)
        if use_async:    # jac_coord! carries the deferred two-way exchange; cons! finds both halos in x
            gm.jac_coord(xd, jv); gm.hess_coord(xd, yd, hv, obj_weight=0.7); gm.cons(xd, c)
        else:
            gm.cons(xd, c); gm.jac_coord(xd, jv); gm.hess_coord(xd, yd, hv, obj_weight=0.7)
        gm.obj_device(xd, f); gm.grad(xd, g)
        gm.allreduce_obj_grad(f, g)
        gm.jtprod(xd, yd, jt)
        gm.halo_fold(jt)
        gm.allreduce_obj_grad(None, jt)

    graph = None
    for it in range(5):
        xg = 0.3 + 0.1 * np.random.default_rng(100 + it).standard_normal(nvg)
        yg = np.random.default_rng(200 + it).standard_normal(ncg)
        xl = xg[vm].copy()
        xl[halo] = np.nan                                  # this rank does NOT hold its neighbours' values
        xd.copy_(torch.tensor(xl)); yd.copy_(torch.tensor(yg[row_map]))
        for out in (c, jv, hv, g, jt):
            out.fill_(float("nan"))
        if use_graph and it >= 2:
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    loop()
            graph.replay()
        else:
            loop()
        torch.cuda.synchronize()
        assert gm.comm_status() == 0, "a mailbox wait timed out"
        xh = xd.cpu().numpy()
        assert np.array_equal(xh[lay.halo_left], xg[vm][lay.halo_left]), "front halo entries differ from the left neighbour's owned values"
        assert np.array_equal(xh[lay.halo_right], xg[vm][lay.halo_right]), "back halo entries differ from the right neighbour's owned values"
        assert np.array_equal(xh, xg[vm])
        sel = owned & ~repl
        res = dict(c=c.cpu().numpy(), j=jv.cpu().numpy(), h=hv.cpu().numpy(), f=f.item(), gown=g.cpu().numpy()[sel], grepl=g.cpu().numpy()[repl],
                   jtown=jt.cpu().numpy()[sel], jtrepl=jt.cpu().numpy()[repl], jthalo=jt.cpu().numpy()[halo],
                   own_idx=vm[sel], repl_idx=vm[repl], row_map=row_map, jpos=jpos, hpos=hpos)
        allres = [None] * world if rank == 0 else None
        dist.gather_object(res, allres, dst=0)
        if rank == 0:
            xgd, ygd = torch.tensor(xg, device="cuda"), torch.tensor(yg, device="cuda")
            cg, jg, hg = (np.full(n, np.nan) for n in (G.meta.ncon, G.meta.nnzj, G.meta.nnzh))
            gg, jtg = np.full(nvg, np.nan), np.full(nvg, np.nan)
            for r in allres:
                cg[r["row_map"]] = r["c"]; jg[r["jpos"]] = r["j"]; hg[r["hpos"]] = r["h"]
                gg[r["own_idx"]] = r["gown"]; gg[r["repl_idx"]] = r["grepl"]
                jtg[r["own_idx"]] = r["jtown"]; jtg[r["repl_idx"]] = r["jtrepl"]
                assert not r["jthalo"].size or not np.any(r["jthalo"]), "halo copies are zeroed by the fold"
                assert r["f"] == allres[0]["f"]
            # the reassembled shard results ARE the one-GPU results, bit for bit
            _same_bits(cg, G.cons(xgd).cpu().numpy(), "cons")
            _same_bits(jg, G.jac_coord(xgd).cpu().numpy(), "jac")
            _same_bits(hg, G.hess_coord(xgd, ygd, obj_weight=0.7).cpu().numpy(), "hess")
            # fold + all-reduce against the unsharded jtprod! / grad! and the oracle, at the suite's bound
            for got, ref, what in ((jtg, G.jtprod(xgd, ygd).cpu().numpy(), "jtprod vs unsharded"), (jtg, O.jtprod(xg, yg), "jtprod"),
                                   (gg, O.grad(xg), "grad"), (cg, O.cons(xg), "cons")):
                scale = np.maximum(np.abs(ref), 1e-10 * max(1.0, np.abs(ref).max()))
                assert (np.abs(got - ref) / scale).max() <= 1e-10, what
            assert abs(allres[0]["f"] - O.obj(xg)) <= 1e-10 * max(1.0, abs(O.obj(xg)))
        dist.barrier()
    if rank == 0:
        print("OK", name, group, world, mode, halo2)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
