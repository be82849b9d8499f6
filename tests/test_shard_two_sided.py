"""Sharding models whose stencils reach to the RIGHT of their support (forward / central differences,
/root/reference/src/transform.jl:535; the heat workload's nested second derivative, transform.jl:141) on CPU: the cut of
`iem_shard_blob` keeps a window with a halo on both sides, flags the copies behind the owned block as the RIGHT
neighbour's (bit 3), and the shards reassemble to the global model; the two-way exchange and its transpose run over the
gloo fallback.  Evaluation by the CPU oracle: this tests the cut and the host plumbing, not the kernels.

tests/golden/shard_cuts/quadrotor_11_w3.npz holds what the commit BEFORE the two-way halo cut out of
`workloads.quadrotor(11)` for the three ranks of world 3 (`lib.shard_blob(blob, 1, r, 3)`: the blob bytes, the flags and
halo / halo_reach / halo_doubles), written from a checkout of that commit with its own library — a left-reaching model
must cut to exactly those bytes."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cases_two_sided as C2
from infiniteexamodels.jl_amd import lib as iemlib, shard, transcribe, workloads
from pyoracle import OracleModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (model, sharded group, world): heat along x (group 2) and along t (group 1); world 8 leaves seven ranks ONE of the 9
# supports of x — fewer than reach_left + reach_right = 2 for central differences
CASES = [("forward_1d", 1, 2), ("forward_1d", 1, 3), ("central_1d", 1, 2), ("central_1d", 1, 3), ("central_1d", 1, 8),
         ("heat_central", 2, 2), ("heat_central", 2, 3), ("heat_central", 2, 8), ("heat_central", 1, 3), ("heat_forward", 2, 8),
         ("heat_forward", 1, 2)]
REACH = {"forward_1d": (0, 1), "central_1d": (1, 1), "heat_central": (1, 1), "heat_forward": (0, 1)}


@pytest.mark.parametrize("name,group,world", CASES)
def test_two_sided_cut_reassembles(name, group, world, built):
    gblob = C2.build_core(name).to_blob()
    G = OracleModel(gblob)
    xg, yg = C2.eval_point(G)
    along_t = name.startswith("heat") and group == 1          # t keeps backward differences
    rl, rr = (1, 0) if along_t else REACH[name]
    c, j, h = (np.full(n, np.nan) for n in (G.ncon, G.nnzj, G.nnzh))
    seen = [np.zeros(n, int) for n in (G.ncon, G.nnzj, G.nnzh)]
    owned = np.zeros(G.nvar, int)
    jt, g = np.zeros(G.nvar), np.zeros(G.nvar)
    f = 0.0
    narrow = False
    for r in range(world):
        cut = iemlib.shard_blob(gblob, group, r, world)
        lblob, info, vm, vf, tpl = cut
        L = OracleModel(lblob)
        lay = shard.ShardLayout.of_cut(cut)
        # --- maps and flags ------------------------------------------------------------------------------
        assert info["halo_reach"] == rl and info["halo"] == (rl if r > 0 else 0)
        assert not ((vf & 1) != 0)[lay.halo].any() and not (lay.halo_left & lay.halo_right).any()
        assert ((vf & 15) != 0).all() and not (vf & ~np.uint8(15)).any(), "every local variable is owned, replicated or a halo copy"
        a, b = shard.partition(info["n_global"], world)[r]
        per = int(lay.halo_left.sum()) // max(info["halo"], 1)          # variables per support of the sharded slabs
        per = per or int(lay.halo_right.sum()) // max(rr, 1) or 0
        want_right = rr if r + 1 < world else 0
        assert info["halo_right_vars"] == int(lay.halo_right.sum())
        if per:
            assert int(lay.halo_right.sum()) == per * want_right and int(lay.halo_left.sum()) == per * info["halo"]
        narrow = narrow or (b - a) < rl + rr
        # halo copies map to variables the neighbour OWNS: front -> rank r - 1, back -> rank r + 1
        for side, nb in ((lay.halo_left, r - 1), (lay.halo_right, r + 1)):
            if side.any():
                nvm, nvf = iemlib.shard_blob(gblob, group, nb, world)[2:4]
                assert np.isin(vm[side], nvm[(nvf & 1) != 0]).all()
        owned[vm[lay.owned & ~lay.replicated]] += 1
        if r == 0:
            owned[vm[lay.replicated]] += 1
        # --- evaluation: bit for bit --------------------------------------------------------------------------
        x, y = xg[vm], yg[lay.row_map]
        c[lay.row_map] = L.cons(x); seen[0][lay.row_map] += 1
        j[lay.jac_pos] = L.jac_coord(x); seen[1][lay.jac_pos] += 1
        h[lay.hess_pos] = L.hess_coord(x, y, 0.7); seen[2][lay.hess_pos] += 1
        f += L.obj(x)
        np.add.at(jt, vm, L.jtprod(x, y))          # what fold + all-reduce compute, in one process
        np.add.at(g, vm, L.grad(x))
        lr, lc = L.jac_structure()
        jr, jc = G.jac_structure()
        assert np.array_equal(lay.row_map[lr], jr[lay.jac_pos]) and np.array_equal(vm[lc], jc[lay.jac_pos])
    assert all((s == 1).all() for s in seen), "every row and COO slot is owned by exactly one rank"
    assert (owned == 1).all(), "every global variable is owned by exactly one rank"
    assert np.array_equal(c, G.cons(xg)) and np.array_equal(j, G.jac_coord(xg)) and np.array_equal(h, G.hess_coord(xg, yg, 0.7))
    assert abs(f - G.obj(xg)) <= 1e-12 * max(1.0, abs(G.obj(xg)))
    np.testing.assert_allclose(jt, G.jtprod(xg, yg), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(g, G.grad(xg), rtol=1e-13, atol=1e-13)
    if (name, group, world) == ("heat_central", 2, 8):   # 9 supports of x over 8 ranks: seven ranks own ONE
        assert narrow, "this case must leave a rank fewer supports than reach_left + reach_right"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("name,group,world", [("central_1d", 1, 2), ("forward_1d", 1, 3), ("heat_central", 2, 3), ("heat_central", 2, 8),
                                              ("heat_central", 1, 2)])
def test_two_way_exchange_and_fold_over_gloo(name, group, world, built):
    """grad! / jtprod! of the shards after the fold and the all-reduce are the global vectors; the exchange fills the halo
    entries on both sides (the torch.distributed fallback of shard.ShardComm, as tests/test_shard.py:104-133 runs it)."""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "shard_two_sided_worker.py"), name, str(group)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    assert "OK" in outs[0], outs[0]


def test_python_transcriber_shards_central_differences(built):
    """The Python re-transcription path (shard.window with a halo on both sides) no longer refuses forward / central
    differences: its central shard evaluates like the C++ cut."""
    world = 3
    gm = C2.ode_1d("central")
    s_global = gm.groups[0].supports[:, 0]
    gblob = transcribe.exa_core(gm).to_blob()
    G = OracleModel(gblob)
    xg, yg = C2.eval_point(G)
    for r in range(world):
        local, f = shard.window(s_global, r, world, halo=1, halo_right=1)
        im = C2.ode_1d("central", supports=local)
        im.shard = shard.ShardSpec(group_index=1, rank=r, world=world, **f)
        P = OracleModel(transcribe.exa_core(im).to_blob())
        lblob, info, vm, vf, tpl = iemlib.shard_blob(gblob, 1, r, world)
        L = OracleModel(lblob)
        assert (P.nvar, P.ncon, P.nnzj, P.nnzh) == (L.nvar, L.ncon, L.nnzj, L.nnzh)
        x = xg[vm]
        y = yg[shard.ShardLayout.of_cut((lblob, info, vm, vf, tpl)).row_map]
        assert np.array_equal(P.cons(x), L.cons(x)) and np.array_equal(P.jac_coord(x), L.jac_coord(x))
        assert np.array_equal(P.hess_coord(x, y, 0.7), L.hess_coord(x, y, 0.7)) and P.obj(x) == L.obj(x)


def test_left_reaching_cut_is_byte_identical_to_the_parent(built):
    """reach_right == 0: the cut, its flags and the front-halo numbers are what they were (see the module docstring)."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "shard_cuts", "quadrotor_11_w3.npz"))
    gblob = transcribe.exa_core(workloads.quadrotor(11)).to_blob()
    for r in range(3):
        lblob, info, vm, vf, tpl = iemlib.shard_blob(gblob, 1, r, 3)
        assert lblob == gold[f"blob_r{r}"].tobytes()
        assert np.array_equal(vf, gold[f"flag_r{r}"]) and not (vf & 8).any() and info["halo_right_vars"] == 0
        assert [info["halo"], info["halo_reach"], info["halo_doubles"]] == gold[f"info_r{r}"].tolist()
        assert info["halo_reach"] == 1 and info["halo"] == (1 if r else 0) and info["halo_doubles"] == 22


@pytest.mark.parametrize("name,group,world", [("heat_central", 2, 3), ("heat_forward", 2, 2), ("central_1d", 1, 3), ("heat_central", 1, 2)])
def test_generated_kernels_of_the_shards_match_the_oracle(name, group, world, built):
    """The GENERATED kernels of every shard (compiled for the host, tests/emu.py), generated as iem_create_sharded does
    (carrier prologue on), write every row and slot and equal the oracle on the same shard.  Heat along x is the case that
    caught a cut bug: the PDE rows are a domain-restricted list the parser recovers as a 2-D box; cut without its grid hint
    it kept the hint's origin and the kernels left its last column unwritten."""
    from types import SimpleNamespace
    from emu import EmulatedModel
    gcore = C2.build_core(name)
    gblob = gcore.to_blob()
    xg, yg = C2.eval_point(OracleModel(gblob))
    for r in range(world):
        cut = iemlib.shard_blob(gblob, group, r, world)
        lay = shard.ShardLayout.of_cut(cut)
        L = OracleModel(cut[0])
        x, y = xg[lay.var_map], yg[lay.row_map]
        with iemlib.options(carrier=1, split_small=0):
            em = EmulatedModel(SimpleNamespace(_blob_arrays=[], theta=gcore.theta), cut[0])   # arrays straight from the shard blob
            c, j, h = em.cons(x), em.jac_coord(x, L.nnzj), em.hess_coord(x, y, 0.7, L.nnzh)
            jt = em.jtprod(x, y)
        rel = lambda a, b: 0.0 if b.size == 0 else float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))
        assert not np.isnan(c).any() and not np.isnan(j).any() and not np.isnan(h).any(), "every output slot must be written"
        assert rel(c, L.cons(x)) <= 1e-14 and rel(j, L.jac_coord(x)) <= 1e-14 and rel(h, L.hess_coord(x, y, 0.7)) <= 1e-14
        assert rel(jt, L.jtprod(x, y)) <= 1e-13
