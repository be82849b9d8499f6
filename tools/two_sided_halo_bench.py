"""Stand-alone time of the halo exchange of a sharded 1-D model, two ranks on ONE GPU (the one-GPU rehearsal bench.py
uses for `comm.halo_exchange_us`, timed the same way: 5 warm-up calls, a barrier, `iters` stream-ordered calls between two
events, the maximum over the ranks).  Models: the finite-difference test ODE with backward (one-way exchange), forward
(one-way, the other direction) and central (two-way) differences at `--supports` supports.

    python tools/two_sided_halo_bench.py --supports 1000000 --iters 200      # prints one JSON line

Rank processes are spawned by the script itself (gloo moves the mailbox handles only)."""
import argparse
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def worker(args):
    import torch
    import torch.distributed as dist
    import cases_two_sided as C2
    from infiniteexamodels.jl_amd import shard, transcribe
    from infiniteexamodels.jl_amd.model import ExaModel
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    out = {}
    for method in args.methods.split(","):
        blob = transcribe.exa_core(C2.ode_1d(method, args.supports)).to_blob()
        gm = ExaModel.sharded(blob, 1, rank, world, device=0, options={"split_small": 0})
        shard.connect_mailboxes(gm, dist)
        x = torch.zeros(gm.meta.nvar, dtype=torch.float64, device="cuda")
        runs = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(5):
                gm.halo_exchange(x)
            dist.barrier(); torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                gm.halo_exchange(x)
            e1.record(); torch.cuda.synchronize()
            t = torch.tensor([e0.elapsed_time(e1) / args.iters * 1e3], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            runs.append(round(float(t.item()), 3))
        assert gm.comm_status() == 0
        out[method] = {"halo_exchange_us": runs, "halo": gm.shard_halo()}
        dist.barrier()
        gm.close()
    if rank == 0:
        print(json.dumps({"supports": args.supports, "world": world, "iters": args.iters, "same_device": True, "models": out}))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supports", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--methods", default="backward,forward,central")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--supports", str(args.supports), "--iters", str(args.iters),
                                       "--repeats", str(args.repeats), "--methods", args.methods], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=900)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        if p.returncode != 0:
            sys.stderr.write(o[-3000:])
            sys.exit(1)
    print([ln for ln in outs[0].splitlines() if ln.startswith("{")][-1])


if __name__ == "__main__":
    main()
