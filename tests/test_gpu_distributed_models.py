"""The wall model and the tabulated streamer on two ranks (two processes on cuda:0 over the host-staged gloo
transport, as tests/test_gpu_distributed.py): streamer_distributed.Runner(model=...).

In each worker, before any step: the global wall state / perturbed state restricted to the rank, one collective
residual() -- the all-reduced fnorm is the norm of the restatement's global F, the owned rows are the restatement's --
then the Jacobian's owned rows and the product behind a halo exchange of its input.  Then two adaptive steps from the
model's initial state: the interior/boundary patch lists with the lazy state halo in between, wall terms that read
ghost potentials; the gathered state is the one-GPU run's of the same model at 1e-8 per component, with the same
Newton iteration count per step.

The global 23 x 23 mesh (n_per_gpu = 16) cuts at constant r under partition_rcb, so each rank holds a part of both
electrodes; the workers assert that instead of trusting the cut.  halo_depth None (eight layers) and 1.
"""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mp_results  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
N_PER_GPU, STEPS, NEQ = 16, 2, 3
TOL = dict(relative_tolerance=1e-8)          # (tests/test_gpu_distributed.py: why not 1e-9)
KRYLOV_RTOL = 1e-11


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _case(name, msh):
    import rank_assembly_reference as rr
    return rr.CASES[name](msh)


def _rel_rows(A, B):
    D = abs(A - B)
    scale = np.maximum(abs(B).max(axis=1).toarray().ravel(), 1e-300)
    return (sp.diags(1.0 / scale) @ D).max()


def _worker(rank, world, port, q, name, halo_depth):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    import rank_assembly_reference as rr
    from fedm_amd.cases import streamer_distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        gmesh, _ = streamer_distributed.global_mesh(N_PER_GPU, world, 2.0)
        c = _case(name, gmesh)
        run = streamer_distributed.Runner(None, rank, world, 0, grading=2.0, transport="torch", n_per_gpu=N_PER_GPU,
                                          halo_depth=halo_depth, model=c["model"](), **TOL)
        run.solver.parameters["krylov_relative_tolerance"] = KRYLOV_RTOL
        prob, lm = run.prob, run.lm
        tags = rr.local_facet_tags(gmesh, lm)
        n_tags = [int((tags == t).sum()) for t in (1, 2)]
        assert min(n_tags) > 0, f"rank {rank} holds no facet of one electrode: {n_tags}"
        # ---- the assembled system of this rank, before any step -----------------------------------------------------
        n_own = lm.n_owned * NEQ
        gdof = (lm.vertex_global[:, None] * NEQ + np.arange(NEQ)[None, :]).ravel()
        F_exp, J_exp, _ = rr.expected_local_system(lm, c["F"], c["J"], NEQ)
        prob.set_state(*[rr.restrict(lm, U) for U in c["states"]])
        prob.set_step(*rr.DT)
        F_gpu, fnorm = prob.residual()
        eF = np.abs(F_gpu[:n_own] - F_exp[:n_own]).max() / np.abs(c["F"]).max()
        prob.jacobian()
        eJ = _rel_rows(prob.jacobian_csr()[:n_own], J_exp[:n_own])
        launched = prob.launched_assembly()
        xg = np.random.default_rng(5).normal(size=c["F"].size)
        x = xg[gdof].copy()
        x[n_own:] = 0.0                                   # the ghost entries come through the halo exchange
        x, _ = prob.comm_roundtrip(x)
        halo_exact = bool(np.array_equal(x, xg[gdof]))
        yc = c["J"] @ xg
        eP = np.abs(prob.spmv(x)[:n_own] - yc[gdof][:n_own]).max() / np.abs(yc).max()
        checks = dict(n_tags=n_tags, eF=float(eF), eJ=float(eJ), eP=float(eP), fnorm=float(fnorm),
                      fnorm_exp=float(np.linalg.norm(c["F"])), halo_exact=halo_exact,
                      variants=(launched["residual"]["variant"], launched["jacobian"]["variant"]),
                      n_ghost=int(lm.n_ghost), depth=int(lm.depth))
        # ---- the solve --------------------------------------------------------------------------------------------
        run.initialise()
        newton = []
        for _ in range(STEPS):
            run.step()
            newton.append(int(prob.last_report.iterations))
        stats = prob.comm_stats()
        checks.update(interior_patches=stats["interior_patches"], boundary_patches=stats["boundary_patches"],
                      halo_exchanges=stats["halo_exchanges"])
        q.put((rank, lm.vertex_global[:lm.n_owned], prob.get_state()[:lm.n_owned], newton, run.log_rows(), checks))
    finally:
        dist.destroy_process_group()


_single = {}


def _single_gpu(name):
    """The one-GPU run of the same model on the whole mesh (once per model)."""
    if name not in _single:
        import rank_assembly_reference as rr
        from fedm_amd.cases import streamer, streamer_distributed
        from fedm_amd.device import DeviceProblem
        from fedm_amd.mesh import Marking_boundaries
        gmesh, n = streamer_distributed.global_mesh(N_PER_GPU, 2, 2.0)
        assert n == 23
        model = _case(name, gmesh)["model"]()
        dofs, vals = streamer.dirichlet(gmesh.coords)
        prob = DeviceProblem(gmesh.coords, gmesh.cells, model, facet_tags=Marking_boundaries(gmesh, streamer.BOUNDARIES),
                             dirichlet_dofs=dofs, dirichlet_vals=vals)
        try:
            st = streamer.Stepper(prob, **TOL)
            st.solver.parameters["krylov_relative_tolerance"] = KRYLOV_RTOL
            st.initialise()
            newton = []
            for _ in range(STEPS):
                st.step()
                newton.append(int(prob.last_report.iterations))
            _single[name] = (prob.get_state(), newton, st.log_rows())
        finally:
            prob.close()
    return _single[name]


@pytest.mark.parametrize("halo_depth", [None, 1])
@pytest.mark.parametrize("name", ["walls", "tabulated"])
def test_two_ranks_assemble_and_solve_as_one_gpu(name, halo_depth):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, name, halo_depth)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(mp_results.collect(procs, q, len(procs), 300), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    U_ref, newton_ref, _ = _single_gpu(name)
    U = np.full_like(U_ref, np.nan)
    for _, gids, Uloc, _, _, _ in res:
        U[gids] = Uloc
    diff = (np.abs(U - U_ref) / np.abs(U_ref).max(axis=0)).max(axis=0)
    for r in res:
        print(f"[two ranks] {name} halo_depth {halo_depth} rank {r[0]}: {r[5]} newton {r[3]}", flush=True)
    print(f"[two ranks] {name} halo_depth {halo_depth}: state diff per component {diff}, one GPU newton {newton_ref}",
          flush=True)
    for r in res:
        k = r[5]
        assert k["depth"] == (8 if halo_depth is None else 1) and k["n_ghost"] > 0
        assert min(k["n_tags"]) > 0
        assert "lds-patches/one-pass" not in k["variants"] and None not in k["variants"]
        assert k["fnorm"] == pytest.approx(k["fnorm_exp"], rel=1e-11)
        assert k["eF"] < 1e-11
        assert k["eJ"] < 1e-10
        assert k["halo_exact"]
        assert k["eP"] < 1e-11
        assert r[3] == newton_ref, (r[3], newton_ref)
    assert diff.max() < 1e-8, diff
