"""Multi-GPU algorithm on ONE GPU: two processes, each with its own context on cuda:0,
talking through the host-staged torch.distributed (gloo) transport.  Everything but the
RCCL calls themselves is the code that runs on 8 GPUs: partition, ghost rows, halo
exchange before SpMV/assembly, all-reduced dots, block-Jacobi/multigrid per rank."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(__import__('pathlib').Path(__file__).resolve().parent))
import mp_results  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
N_PER_GPU, STEPS = 16, 3
# Newton's relative tolerance of these comparisons.  It was 1e-9 until a step of the two-rank run failed once in ~25
# runs: "maximum number of Newton iterations reached" at |F| = 4.07e5 from |F0| = 2.13e14, i.e. the residual stalls at
# 1.9e-9 |F0| -- the rounding floor of the assembled residual (sums of 1e14-sized terms in an order the LDS atomics do
# not fix) sits ABOVE 1e-9 |F0| in some runs; adaptive_solver then halves the step and the histories differ.  1e-8 is
# five times that floor; the states still agree to 1e-8 x (a step's change) << the 1e-8 asked of them below.
TOL = dict(relative_tolerance=1e-8)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q, restart=30, halo_depth=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    from fedm_amd.cases import streamer, streamer_distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        run = streamer_distributed.Runner(None, rank, world, 0, grading=2.0, transport="torch",
                                          n_per_gpu=N_PER_GPU, halo_depth=halo_depth, **TOL)
        run.solver.parameters["krylov_relative_tolerance"] = 1e-11
        run.solver.parameters["krylov_restart"] = restart
        run.initialise()
        raised, solve = [], run.solver.solve      # (what adaptive_solver's catch-all swallows, for the failure message)

        def logged(*a, **k):
            try:
                return solve(*a, **k)
            except Exception as e:
                raised.append((repr(e), run.prob.last_report))
                raise
        run.solver.solve = logged
        for _ in range(STEPS):
            run.step()
        U = run.prob.get_state()[:run.lm.n_owned]
        stats = run.prob.comm_stats()
        q.put((rank, run.lm.vertex_global[:run.lm.n_owned], U, run.log_rows(), run.global_n,
               (stats["halo_exchanges"], stats["allreduces"], run.linear_iterations, int(run.lm.n_ghost),
                run.prob.fieldsplit_tiles() is not None, [str(r) for r in raised])))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("restart,halo_depth,partitioner", [(30, None, "rcb"), (3, None, "rcb"), (30, 1, "rcb"), (30, 3, "rcb"),
                                                            (30, None, "graph")])
def test_two_ranks_match_single_gpu(restart, halo_depth, partitioner, monkeypatch):
    """restart = 3 makes every linear solve run through several GMRES cycles: the restarted
    residual rhs - J delta (halo exchange of delta, plain product) and the accumulated update.
    halo_depth: None = the default of eight ghost layers (one exchange per Krylov step: the input
    vector on all layers; sweeps, smoothings and product on redundantly assembled ghost rows),
    1 = the one-layer halo with an exchange before every operator, 3 = ghost layers that do NOT
    cover a preconditioner application (the library must fall back to the exchanges).  partitioner: the coordinate
    bisection, or the multilevel graph partitioner (FEDM_PARTITIONER=graph, fedm_amd/graph_partition.py)."""
    import torch.multiprocessing as mp
    from fedm_amd.cases import streamer
    monkeypatch.setenv("FEDM_PARTITIONER", partitioner)     # (the spawned ranks inherit it)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, restart, halo_depth)) for r in range(2)]
    for p in procs:
        p.start()
    res = mp_results.collect(procs, q, len(procs), 300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n = res[0][4]
    msh = streamer.mesh(n, 2.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    st = streamer.Stepper(prob, **TOL)
    st.solver.parameters["krylov_relative_tolerance"] = 1e-11
    st.initialise()
    for _ in range(STEPS):
        st.step()
    U_ref = prob.get_state()
    U = np.zeros_like(U_ref)
    for _, gids, Uloc, _, _, _ in res:
        U[gids] = Uloc
    scale = np.abs(U_ref).max(axis=0)
    diff = (np.abs(U - U_ref) / scale).max()
    if diff >= 1e-8:        # (what a failure is made of, in full: pytest shortens assertion messages)
        print("per-field max |U - U_ref|:", np.abs(U - U_ref).max(axis=0), "mean signed:", (U - U_ref).mean(axis=0))
        print("two ranks: log", res[0][3], "stats", res[0][5], "| rank 1 log", res[1][3], "stats", res[1][5])
        print("one GPU: log", st.log_rows(), "newton", st.newton_iterations, "krylov", st.linear_iterations)
    assert diff < 1e-8, diff
    ref_log = np.array(st.log_rows())
    for r in res:
        assert np.allclose(np.array(r[3]), ref_log, rtol=1e-6)
    # the deep halo saves the exchanges (Krylov counts at this 1e-11 tolerance end in rounding and vary by tens
    # of per cent between any two runs; at the default tolerances they are those of one GPU: tools/rehearse_multi_rank.sh)
    halos, _, krylov, n_ghost, tiled = res[0][5][:5]
    # deep halos: nothing is exchanged between the species sweeps, so they run several per launch on tiles as on
    # one GPU (csrc/fs_tiles.hip); with an exchange before every sweep they cannot
    assert tiled == (halo_depth is None)
    if restart == 30:
        if halo_depth is None:
            assert halos < 3 * krylov            # ~1.5 per Krylov step (its input + the state halos)
        else:
            assert halos > 6 * krylov            # an exchange before every sweep, smoothing and product


def test_rccl_transport_single_rank():
    """RCCL is resolved with dlopen and driven on the library's stream: a one-rank
    communicator (self all-reduce, empty halo) must not change the solve."""
    from fedm_amd import partition
    from fedm_amd.cases import streamer
    from fedm_amd.device import rccl_unique_id
    msh = streamer.mesh(16, 2.0)
    part = partition.partition_rcb(msh.coords, 1)
    lm = partition.local_mesh(msh.coords, msh.cells, part, 0)
    assert lm.n_ghost == 0 and len(lm.neighbours) == 0
    out = []
    for use_rccl in (False, True):
        prob = streamer.device_problem(msh.coords, msh.cells)
        if use_rccl:
            prob.init_comm_rccl(lm, rccl_unique_id(), 0, 1)
        st = streamer.Stepper(prob)
        st.initialise()
        st.step()
        out.append(prob.get_state())
        prob.close()
    # not bitwise: the LDS-atomic assembly sums in a run-dependent order
    assert np.allclose(out[0], out[1], rtol=1e-9, atol=1e-9)


def test_rccl_point_to_point_path_on_one_rank_that_is_its_own_neighbour():
    """ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd and ncclAllReduce as the halo code issues them,
    on real RCCL with ONE rank: the sub-mesh of rank 0 of a two-way partition, with the exchange plan
    rewired so that the rank sends the values of some owned vertices to itself and receives them into
    its ghost segment (RCCL allows a send to self inside a group).  Not a meaningful solve -- the data
    path of the transport by itself, which two ranks on one GPU cannot exercise (RCCL refuses them)."""
    import dataclasses
    from fedm_amd import partition
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, rccl_unique_id
    msh = streamer.mesh(24, 2.0)
    part = partition.partition_rcb(msh.coords, 2)
    lm = partition.local_mesh(msh.coords, msh.cells, part, 0)
    n_ghost = lm.n_ghost
    assert n_ghost > 0 and n_ghost <= lm.n_owned
    rng = np.random.default_rng(5)
    send = np.sort(rng.choice(lm.n_owned, size=n_ghost, replace=False))
    me = dataclasses.replace(lm, neighbours=np.array([0]), send_ptr=np.array([0, n_ghost]), send_idx=send,
                             recv_ptr=np.array([0, n_ghost]))
    tags = np.zeros((lm.cells.shape[0], 3), dtype=np.int8)
    prob = DeviceProblem(lm.coords, lm.cells, streamer.model(), facet_tags=tags, n_owned=lm.n_owned)
    try:
        prob.init_comm_rccl(me, rccl_unique_id(), 0, 1)
        neq = prob.n_eq
        v = rng.standard_normal((prob.nv, neq))
        v[lm.n_owned:] = 0.0
        out, red = prob.comm_roundtrip(v.ravel(), red=[1.5, -2.0, 3.25])
        out = out.reshape(prob.nv, neq)
        assert np.array_equal(out[:lm.n_owned], v[:lm.n_owned])          # owned entries untouched
        assert np.array_equal(out[lm.n_owned:], v[send])                 # ghosts = what was "sent"
        assert np.array_equal(red, [1.5, -2.0, 3.25])                    # a sum over one rank
        stats = prob.comm_stats()
        assert stats["transport"] == "rccl" and not stats["failed"] and stats["halo_exchanges"] >= 1
    finally:
        prob.close()


def _worker_rccl(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    from fedm_amd.cases import streamer_distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        run = streamer_distributed.Runner(None, rank, world, 0, grading=2.0, transport="rccl",
                                          n_per_gpu=N_PER_GPU)
        run.initialise()
        run.step()
        q.put((rank, run.partition_name, run.linear_iterations))
    finally:
        dist.destroy_process_group()


def test_rccl_setup_failure_falls_back_on_every_rank():
    """Two ranks on ONE device: the RCCL bootstrap between the processes works, then RCCL refuses
    the duplicate GPU.  All ranks must agree on that and continue over the host-staged transport
    (the scaling runs must not die on a transport problem)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_rccl, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = mp_results.collect(procs, q, len(procs), 300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all("RCCL set-up failed" in r[1] for r in res)
    assert res[0][2] == res[1][2] > 0


def _worker_galerkin(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import scipy.sparse as sp
    import torch.distributed as dist
    from fedm_amd import amg
    from fedm_amd.cases import streamer_distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        run = streamer_distributed.Runner(None, rank, world, 0, grading=2.0, transport="torch",
                                          n_per_gpu=N_PER_GPU)
        prob, lm = run.prob, run.lm
        seen = {}
        original = amg.install

        def spy(handle, levels, **kw):                 # the finest level as it goes to the device
            seen["levels"] = levels
            return original(handle, levels, **kw)
        amg.install = spy
        run.initialise()
        (K_dev, P_dev), (A1, _) = seen["levels"]
        n_own, gid = lm.n_owned, lm.vertex_global
        K_rows = sp.csr_matrix(K_dev)[prob._inv][:, prob._inv][:n_own].tocoo()     # local numbering
        P_rows = sp.csr_matrix(P_dev)[prob._inv][:n_own].tocoo()                    # global columns
        gathered = [None] * world
        dist.all_gather_object(gathered, dict(gid=gid, n_own=n_own, K=K_rows, P=P_rows, A1=A1 if rank == 0 else None))
        if rank == 0:
            nvg = max(int(g["gid"].max()) for g in gathered) + 1
            n_g = A1.shape[0]
            kr, kc, kv, pr, pc, pv = [], [], [], [], [], []
            for g in gathered:
                own = g["gid"][:g["n_own"]]
                kr.append(own[g["K"].row]); kc.append(g["gid"][g["K"].col]); kv.append(g["K"].data)
                pr.append(own[g["P"].row]); pc.append(g["P"].col); pv.append(g["P"].data)
            Kg = sp.csr_matrix((np.concatenate(kv), (np.concatenate(kr), np.concatenate(kc))), shape=(nvg, nvg))
            Pg = sp.csr_matrix((np.concatenate(pv), (np.concatenate(pr), np.concatenate(pc))), shape=(nvg, n_g))
            ref = (Pg.T @ Kg @ Pg).toarray()
            ones = np.asarray(Pg.sum(axis=1)).ravel()
            offdiag = np.asarray(abs(Kg).sum(axis=1)).ravel() - abs(Kg.diagonal())
            dirichlet = (offdiag == 0.0).astype(np.float64)                 # identity rows
            away = (dirichlet == 0.0) & (np.asarray(abs(Kg) @ dirichlet).ravel() == 0.0)
            q.put(("A1 max abs diff", float(np.abs(ref - A1.toarray()).max()), "scale", float(np.abs(ref).max()),
                   "asym of ref", float(np.abs(ref - ref.T).max()),
                   "row sums of P off 1", float(np.abs(ones[away] - 1.0).max())))
    finally:
        dist.destroy_process_group()


def test_distributed_galerkin_operator_is_the_global_one():
    """The level-1 operator of the multi-GPU multigrid is the sum of the ranks' contributions
    (owned rows of K x prolongator rows, the ghost vertices' rows fetched from the neighbours).
    It must equal P^T K P of the undecomposed block, formed here directly from the gathered
    pieces, and the prolongator -- smoothed with the undecomposed operator -- must reproduce
    constants across the partition boundary."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_galerkin, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = mp_results.collect(procs, q, 1, 300)[0]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    diff, scale, asym, rowsum = res[1], res[3], res[5], res[7]
    assert diff < 1e-13 * scale and asym < 1e-13 * scale
    assert rowsum < 1e-12


def test_bench_multi_rank_path_end_to_end():
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one JSON line from
    rank 0), rehearsed with two ranks on this one GPU: gloo process group, RCCL set-up refused for
    the duplicate device, host-staged transport."""
    import json
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(ROOT / "bench.py"),
           "--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--mesh", "64", "--rehearse-on-one-gpu",
           "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 2 and res["scaling"] == "weak"
    assert res["value"] > 0 and res["unit"] == "DOF-updates/s"
    assert res["config"]["dofs_total"] > 2 * 64 * 64 * 3 * 0.9
    assert {"roofline", "cpu_baseline", "ms_per_step", "metric"} <= set(res)


def _worker_rccl_two_devices(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch
    import torch.distributed as dist
    from fedm_amd.cases import streamer_distributed
    torch.cuda.set_device(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        run = streamer_distributed.Runner(None, rank, world, rank, grading=2.0, transport="rccl",
                                          n_per_gpu=N_PER_GPU, distributed_multigrid=True, **TOL)
        run.solver.parameters["krylov_relative_tolerance"] = 1e-11
        run.initialise()
        for _ in range(STEPS):
            run.step()
        U = run.prob.get_state()[:run.lm.n_owned]
        q.put((rank, run.lm.vertex_global[:run.lm.n_owned], U, run.log_rows(), run.global_n, run.transport,
               run.prob.comm_stats()))
    finally:
        dist.destroy_process_group()


def test_several_gpu_solver_on_one_rank_over_rccl_matches_single_gpu():
    """The whole several-GPU solver on real RCCL with ONE rank: distributed finest multigrid level,
    replicated coarse levels with their (single-precision payload) all-reduce, the Krylov loop with its
    halo / all-reduce / finish sequence and split graphs -- everything but a second process.  Same
    time steps as the plain single-GPU solver."""
    import torch.multiprocessing as mp
    from fedm_amd.cases import streamer
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker_rccl_two_devices, args=(0, 1, _free_port(), q))
    p.start()
    res = mp_results.collect([p], q, 1, 600)[0]
    p.join(timeout=60)
    assert p.exitcode == 0, p.exitcode
    assert res[5] == "rccl" and res[6]["transport"] == "rccl" and not res[6]["failed"] and res[6]["allreduces"] > 0, (res[5], res[6])
    msh = streamer.mesh(res[4], 2.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    st = streamer.Stepper(prob, **TOL)
    st.solver.parameters["krylov_relative_tolerance"] = 1e-11
    st.initialise()
    for _ in range(STEPS):
        st.step()
    U_ref = prob.get_state()
    U = np.zeros_like(U_ref)
    U[res[1]] = res[2]
    diff = (np.abs(U - U_ref) / np.abs(U_ref).max(axis=0)).max()
    assert diff < 1e-8, (diff, res[3], st.log_rows())


def test_two_ranks_over_rccl_match_single_gpu():
    """The RCCL data path itself (ncclSend/ncclRecv halo groups, ncclAllReduce, the state halo
    behind interior assembly patches) between two processes on two GPUs.  Needs two devices: on
    the one-GPU boxes of the development pool it is skipped, and the same algorithm is covered over
    the host-staged transport above."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import torch.multiprocessing as mp
    from fedm_amd.cases import streamer
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_rccl_two_devices, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = mp_results.collect(procs, q, len(procs), 600)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[5] == "rccl" and r[6]["transport"] == "rccl" and not r[6]["failed"] for r in res)
    assert all(r[6]["halo_exchanges"] > 0 and r[6]["allreduces"] > 0 for r in res)
    n = res[0][4]
    msh = streamer.mesh(n, 2.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    st = streamer.Stepper(prob, **TOL)
    st.solver.parameters["krylov_relative_tolerance"] = 1e-11
    st.initialise()
    for _ in range(STEPS):
        st.step()
    U_ref = prob.get_state()
    U = np.zeros_like(U_ref)
    for r in res:
        U[r[1]] = r[2]
    assert (np.abs(U - U_ref) / np.abs(U_ref).max(axis=0)).max() < 1e-8


def test_state_halo_behind_interior_assembly_is_the_same_solve(monkeypatch):
    """FEDM_ASSEMBLY_OVERLAP=0 exchanges the ghost values of the new state on the compute stream
    before the assembly; the default sends them on the communication stream while the interior
    patches (those that stage no ghost vertex) are assembled.  Same time steps either way."""
    import torch.multiprocessing as mp
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("FEDM_ASSEMBLY_OVERLAP", flag)
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = sorted(mp_results.collect(procs, q, len(procs), 300), key=lambda r: r[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        out[flag] = res
    for a, b in zip(out["1"], out["0"]):
        assert np.array_equal(a[1], b[1])
        assert np.allclose(a[2], b[2], rtol=1e-9, atol=1e-9)
        assert np.allclose(np.array(a[3]), np.array(b[3]), rtol=1e-7)
