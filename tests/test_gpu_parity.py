"""GPU parity: the HIP path (through the C ABI) against the oracle and the goldens.

fp64 throughout.  Tolerances: element-level quantities (residual, Jacobian,
SpMV) 1e-11 relative to the row/vector scale -- the kernel sums the same terms
in a different association; solver-level quantities are bounded by the
solvers' own stopping tolerances and stated per test.
"""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def streamer_setup():
    from oracle import streamer as ost
    from oracle.mesh import graded_axis, rectangle_right
    from fedm_amd.cases import streamer
    n = 20
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, n, n, xs=graded_axis(ost.BOX, n, 6.0))
    omodel = ost.build(mesh)
    U0 = ost.initial_state(omodel)
    prob = streamer.device_problem(mesh.coords, mesh.cells)
    return mesh, omodel, U0, prob


def _perturbed(U0, seed):
    rng = np.random.default_rng(seed)
    U = U0.copy()
    U[:, 0] += rng.normal(0, 0.05, U.shape[0])
    U[:, 1] += rng.normal(0, 0.3, U.shape[0])
    U[:, 2] += rng.normal(0, 20.0, U.shape[0])
    return U


def _rel_rows(A, B):
    D = abs(A - B)
    scale = np.maximum(abs(B).max(axis=1).toarray().ravel(), 1e-300)
    return (sp.diags(1.0 / scale) @ D).max()


@pytest.mark.parametrize("dt,dt_old", [(5e-12, 1e30), (5e-12, 4e-12)])
def test_streamer_residual_and_jacobian(streamer_setup, dt, dt_old):
    mesh, omodel, U0, prob = streamer_setup
    U, Uo, Uo1 = _perturbed(U0, 1), _perturbed(U0, 2), _perturbed(U0, 3)
    prob.set_state(U, Uo, Uo1)
    prob.set_step(dt, dt_old)
    F_gpu, fnorm = prob.residual()
    F_cpu, J_cpu = omodel.residual_jacobian(U, Uo, Uo1, dt, dt_old)
    scale = np.abs(F_cpu).max()
    assert np.abs(F_gpu - F_cpu).max() / scale < 1e-11
    assert fnorm == pytest.approx(np.linalg.norm(F_cpu), rel=1e-11)
    prob.jacobian()
    J_gpu = prob.jacobian_csr()
    assert _rel_rows(J_gpu, J_cpu) < 1e-10
    # structural check: same pattern up to explicit zeros
    assert (abs(J_gpu) > 0).sum() <= J_gpu.nnz
    x = np.random.default_rng(5).normal(size=prob.n)
    y = prob.spmv(x)
    yc = J_cpu @ x
    assert np.abs(y - yc).max() / np.abs(yc).max() < 1e-11


def test_streamer_poisson_solve(streamer_setup):
    mesh, omodel, U0, prob = streamer_setup
    U = U0.copy()
    U[:, 2] = 0.0
    prob.set_state(U, U, U)
    its = prob.poisson_solve(rtol=1e-13)
    Phi = prob.get_state()[:, 2]
    assert its > 0
    assert np.abs(Phi - U0[:, 2]).max() / np.abs(U0[:, 2]).max() < 1e-9


def test_streamer_newton_step(streamer_setup):
    from oracle.newton import newton_solve
    mesh, omodel, U0, prob = streamer_setup
    prob.set_state(U0, U0, U0)
    prob.set_step(5e-12, 1e30)
    its, _ = prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    U_gpu = prob.get_state()
    U_cpu = U0.copy()
    its_cpu, _ = newton_solve(omodel, U_cpu, U0, U0, 5e-12, 1e30, 1e-8, 20)
    assert its == its_cpu
    d = np.abs(U_gpu - U_cpu).max(axis=0) / np.abs(U_cpu).max(axis=0)
    assert d.max() < 1e-9
    e_gpu = prob.field_error(1)   # u_old on the device is still U0
    from oracle.controller import field_error
    assert e_gpu == pytest.approx(field_error(U_cpu[:, 1], U0[:, 1]), rel=1e-7)


def test_streamer_error_log(streamer_setup):
    """Five adaptive steps: the device path reproduces the oracle's error log rows."""
    from oracle import streamer as ost
    from fedm_amd.cases import streamer
    from fedm_amd import functions as ff
    mesh, omodel, U0, prob = streamer_setup
    _, st, _, _ = ost.run(mesh=mesh, max_steps=5)
    rows = streamer.run(prob, max_steps=5)["log"]
    assert len(rows) == len(st.log)
    assert np.allclose(np.array(rows), np.array(st.log), rtol=2e-4)


def test_tof_residual_and_jacobian():
    from oracle import tof as otof
    from oracle.forms import LFAModel
    from oracle.mesh import rectangle_right
    from fedm_amd.cases import time_of_flight as tof
    nx = ny = 12
    prob, mesh = tof.device_problem(nx, ny, 2.5e-4, 5e-4)
    omesh = rectangle_right(0, 0, 2.5e-4, 5e-4, nx, ny)
    om = LFAModel(omesh, 1, False, ["drift-diffusion-reaction"], [-1.0], D=[otof.DE],
                  drift_w=[(0.0, otof.WEZ)], qdeg=8)
    t0, dt = 2.5e-9, 1e-12
    rng = np.random.default_rng(0)
    U = otof.log_density(omesh.coords, t0, 3e-16)[:, None] + rng.normal(0, 0.1, (omesh.nv, 1))
    Uo = otof.log_density(omesh.coords, t0)[:, None]
    Uo1 = Uo + rng.normal(0, 0.1, (omesh.nv, 1))
    src = otof.source(otof.cell_nodes(omesh, 2), t0 + dt)
    assert np.allclose(tof.p2_nodes(mesh.coords, mesh.cells), otof.cell_nodes(omesh, 2))
    om.set_ext_source(0, 2, src)
    prob.set_ext_source(0, tof.source(tof.p2_nodes(mesh.coords, mesh.cells), t0 + dt))
    for dt_old in (1e30, 2e-12):
        prob.set_state(U, Uo, Uo1)
        prob.set_step(dt, dt_old)
        F_gpu, _ = prob.residual()
        F_cpu, J_cpu = om.residual_jacobian(U, Uo, Uo1, dt, dt_old)
        assert np.abs(F_gpu - F_cpu).max() / np.abs(F_cpu).max() < 1e-11
        prob.jacobian()
        assert _rel_rows(prob.jacobian_csr(), J_cpu) < 1e-10


def test_tof_golden(golden_dir):
    """The reference's own ToF test (test_time_of_flight.py:45-56) on the device path."""
    from fedm_amd.cases import time_of_flight as tof
    gold = np.load(golden_dir / "tof_golden.npz")
    out = tof.run_harness()
    assert np.isclose(out["relative_error"], float(gold["relative_error"]))
    err = (out["n_num"] - gold["n_e"]) / gold["n_e"]
    assert np.mean(np.abs(err)) < 1e-5
    assert np.sqrt(np.mean(err ** 2)) < 1e-5
    assert np.max(np.abs(err)) < 1e-3


def test_tof_example_script_reproduces_the_golden(golden_dir, tmp_path):
    """examples/time_of_flight.py -- our own driver for the case of fedm-tof.py (C++ Expression strings,
    the flux written by hand, PETScSNESSolver driven by the script; tests/test_reference_scripts.py shows
    that it hands the device what the reference's script does) -- with the harness's sizes
    (tests/integrated_tests/time_of_flight/fedm_tof.py: 40x40, 100 steps) against the same golden."""
    import importlib.util
    from fedm_amd.cases import time_of_flight as tof
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("tof_example", root / "examples" / "time_of_flight.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gold = np.load(golden_dir / "tof_golden.npz")
    n_num, n_exact, rel = mod.main(nx=40, ny=40, box_width=2.5e-4, box_height=5e-4, t0=2.5e-9,
                                   T_final=2.6e-9, t_output=2.6e-9, output_dir=tmp_path, quiet=True)
    assert np.isclose(rel, float(gold["relative_error"]))
    err = (n_num - gold["n_e"]) / gold["n_e"]
    assert np.mean(np.abs(err)) < 1e-5 and np.sqrt(np.mean(err ** 2)) < 1e-5 and np.max(np.abs(err)) < 1e-3
    direct = tof.run_harness()                       # the case module, without the facade
    assert np.abs(n_num - direct["n_num"]).max() <= 1e-9 * np.abs(direct["n_num"]).max()
    assert np.abs(n_exact - direct["n_exact"]).max() <= 1e-12 * np.abs(direct["n_exact"]).max()


def test_expression_source_evaluated_on_the_device_matches_the_host():
    """fedm_ext_source_program / fedm_ext_source_eval: the postfix program of the ToF source string, run
    by the device at the P2 lattice nodes of every cell, against the host evaluation of the same string
    uploaded with fedm_set_ext_source -- through the residual, which is where the table is used."""
    from fedm_amd import forms
    from fedm_amd.cases import time_of_flight as tof
    prob, mesh = tof.device_problem(24, 32, 2.5e-4, 5e-4)
    f = forms.Expression('exp(-(pow(x[1]-w*t, 2)+pow(x[0], 2))/(4.0*D*t)+alpha*w*t)*(w*alpha)'
                         '/(8*pow(pi,1.5)*pow(D*t, 1.5))', D=tof.DE, w=tof.WEZ, alpha=tof.ALPHA_E, t=2.5e-9,
                         pi=np.pi, degree=2)
    ops, consts, names = forms.expression_program(f)
    prob.set_ext_source_program(0, ops, consts, len(names))
    u = tof.analytic_log_density(mesh.coords, 2.5e-9)
    prob.set_state(u, u, u)
    prob.set_step(1e-12, 1e30)
    nodes = tof.p2_nodes(mesh.coords, mesh.cells)
    for t in (2.5e-9, 2.6e-9):
        f.t = t
        prob.set_ext_source(0, np.asarray(f(nodes)))
        F_host, _ = prob.residual()
        prob.set_ext_source(0, np.zeros(nodes.shape[:2]))
        F_none, _ = prob.residual()
        prob.eval_ext_source(0, [getattr(f, n) for n in names])
        F_dev, _ = prob.residual()
        scale = np.abs(F_host - F_none).max()
        assert scale > 0 and np.abs(F_dev - F_host).max() <= 1e-12 * scale      # exp / pow differ by ulps
    with pytest.raises(RuntimeError, match="bad expression program"):
        prob.set_ext_source_program(0, [[3, 0]], [], 0)                         # an operator on an empty stack
    with pytest.raises(RuntimeError, match="bad expression program"):
        prob.set_ext_source_program(0, [[0, 2]], [1.0], 0)                      # constant index out of range


def test_streamer_multigrid_fieldsplit(streamer_setup):
    """Field-split + V-cycle preconditioning changes the Krylov path, not the answer."""
    from oracle.newton import newton_solve
    mesh, omodel, U0, prob = streamer_setup
    levels = prob.setup_multigrid(max_coarse=40)
    assert len(levels) >= 2
    try:
        U = U0.copy()
        U[:, 2] = 0.0
        prob.set_state(U, U, U)
        its_cg = prob.poisson_solve(rtol=1e-13)
        Phi = prob.get_state()[:, 2]
        assert its_cg < 40
        assert np.abs(Phi - U0[:, 2]).max() / np.abs(U0[:, 2]).max() < 1e-9
        prob.set_state(U0, U0, U0)
        prob.set_step(5e-12, 1e30)
        prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
        lin_amg = prob.last_report.linear_iterations
        U_gpu = prob.get_state()
        U_cpu = U0.copy()
        newton_solve(omodel, U_cpu, U0, U0, 5e-12, 1e30, 1e-8, 20)
        d = np.abs(U_gpu - U_cpu).max(axis=0) / np.abs(U_cpu).max(axis=0)
        assert d.max() < 1e-9
    finally:
        prob.clear_multigrid()
    prob.set_state(U0, U0, U0)
    prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    assert lin_amg < prob.last_report.linear_iterations


def test_single_precision_hierarchy_is_the_same_preconditioner(streamer_setup, monkeypatch):
    """The multigrid matrices are stored in single precision (EllMat::single; vectors and sums are
    double): against the double-precision hierarchy (FEDM_MG_F32=0) the Poisson-only CG takes the same
    number of iterations, and both it and the Newton solve end in the same states."""
    mesh, omodel, U0, prob = streamer_setup
    out = {}
    for tag, env in (("single", "1"), ("double", "0")):
        monkeypatch.setenv("FEDM_MG_F32", env)
        prob.setup_multigrid(max_coarse=40)
        try:
            U = U0.copy()
            U[:, 2] = 0.0
            prob.set_state(U, U, U)
            its_cg = prob.poisson_solve(rtol=1e-13)
            phi = prob.get_state()[:, 2]
            prob.set_state(U0, U0, U0)
            prob.set_step(5e-12, 1e30)
            prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
            out[tag] = (its_cg, phi, prob.last_report.linear_iterations, prob.get_state())
        finally:
            prob.clear_multigrid()
    a, b = out["single"], out["double"]
    assert abs(a[0] - b[0]) <= 1          # (Krylov counts of the Newton systems also depend on what the
    #                                        solver has adapted to before: bench.py reports them, 6.0 / 26.1)
    assert np.abs(a[1] - b[1]).max() <= 1e-10 * np.abs(b[1]).max()
    assert (np.abs(a[3] - b[3]).max(axis=0) / np.abs(b[3]).max(axis=0)).max() < 1e-9


def test_example_script_in_fedm_shape(tmp_path):
    """examples/streamer_discharge.py (our own driver for the case of fedm-streamer.py on the
    fedm.functions façade) gives the same error log as the case module on the same mesh -- on the graded
    tensor-product mesh and on the locally refined unstructured mesh it writes to and loads from
    `mesh.xml` like the reference's script loads its mesh."""
    import importlib.util
    from pathlib import Path
    from fedm_amd.cases import streamer
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("ex_streamer", root / "examples" / "streamer_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    state, log = mod.main(cells=24, end_time=2e-11, output_dir=tmp_path, quiet=True)
    rows = np.loadtxt(log).reshape(-1, 3)
    msh = streamer.mesh(24, 4.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    ref = streamer.run(prob, T_final=2e-11)
    assert rows.shape == (4, 3) and np.allclose(rows, np.array(ref["log"]), rtol=1e-6)
    assert np.allclose(state, prob.get_state(), rtol=1e-8, atol=1e-8)
    prob.close()
    state, log = mod.main(mesh_spacing=60e-6, end_time=2e-11, output_dir=tmp_path / "unstructured", quiet=True)
    rows = np.loadtxt(log).reshape(-1, 3)
    from fedm_amd import mesh_io
    msh = mesh_io.read_dolfin_xml(tmp_path / "unstructured" / "mesh" / "mesh.xml")
    assert msh.num_vertices() == state.shape[0] > 4000
    prob = streamer.device_problem(msh.coords, msh.cells)
    ref = streamer.run(prob, T_final=2e-11)
    assert rows.shape == (4, 3) and np.allclose(rows, np.array(ref["log"]), rtol=1e-5)
    # (two Newton solves to rtol 1e-4 with different multigrid set-ups: agreement within that tolerance)
    assert np.allclose(state, prob.get_state(), rtol=1e-5, atol=1e-6)
    prob.close()


def test_krylov_graphs_match_plain_launches():
    """GMRES replays one captured hipGraph per Krylov index and finishes the field split inside
    its reduction kernel; with kernel profiling on it launches the same kernels one by one.
    Same arithmetic, same order: iteration counts and states must agree."""
    from fedm_amd.cases import streamer
    msh = streamer.mesh(48, 4.0)
    out = {}
    for mode in ("graphs", "plain"):
        prob = streamer.device_problem(msh.coords, msh.cells)
        st = streamer.Stepper(prob)
        st.initialise()
        if mode == "plain":
            prob.profile(2)
        counts = []
        for _ in range(3):
            l0, n0 = st.linear_iterations, st.newton_iterations
            st.step()
            counts.append((st.newton_iterations - n0, st.linear_iterations - l0))
        out[mode] = (counts, prob.get_state())
        if mode == "plain":
            assert prob.profile_read()["spmv"][1] > 0      # the profiled kinds were really timed
        prob.close()
    assert out["graphs"][0] == out["plain"][0]
    assert np.allclose(out["graphs"][1], out["plain"][1], rtol=1e-10, atol=1e-10)


def test_composite_multigrid_levels_are_the_same_cycle(monkeypatch):
    """Below the finest level the V(1,1) cycle runs two precomputed products per level
    (b_c = R(I - wA Dinv) b and x = G b + Q x_c) instead of sweep, restriction, prolongation, sweep.
    The same linear operator: the Poisson CG and the time steps must not notice."""
    from fedm_amd.cases import streamer
    msh = streamer.mesh(128, 4.0)
    out = {}
    for composite in ("0", "1"):
        monkeypatch.setenv("FEDM_AMG_COMPOSITE", composite)
        prob = streamer.device_problem(msh.coords, msh.cells)
        st = streamer.Stepper(prob)
        _, its = st.initialise()
        assert len(prob.multigrid_levels) >= 3          # at least one composite level
        for _ in range(2):
            st.step()
        out[composite] = (its, st.linear_iterations, prob.get_state())
        prob.close()
    assert out["0"][0] == out["1"][0] and out["0"][1] == out["1"][1]
    assert np.allclose(out["0"][2], out["1"][2], rtol=1e-9, atol=1e-9)


def test_polynomial_smoother_cycle_is_the_richardson_cycle_and_contracts_faster():
    """fedm_amg_setup_poly folds k Richardson sweeps per leg into the composite products of the
    coarse levels and into [S | P] on the finest one.  With one sweep of weight w it is the V(1,1)
    cycle with damping w (same CG count, same solution); with two Chebyshev sweeps the Poisson-only
    CG needs fewer steps and reaches the same potential; installed as the alternative for hard
    systems it leaves the trajectory of the time steps alone."""
    from fedm_amd import amg
    from fedm_amd.cases import streamer
    msh = streamer.mesh(128, 4.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    U0 = np.zeros((prob.nv, 3))
    U0[:, 0], U0[:, 1] = streamer.initial_log_densities(prob.coords)

    def poisson(install):
        prob.set_state(U0, U0, U0)
        install()
        its = prob.poisson_solve(rtol=1e-12)
        return its, prob.get_state()[:, 2].copy()

    def poly(degree, weights=None):
        def f():
            prob.setup_multigrid(nu=1, omega=0.85)                       # builds the hierarchy ...
            levels = prob._last_hierarchy
            amg.install_poly(prob._h, levels, degree, weights=weights)   # ... installed with the polynomial
        return f
    its_v, phi_v = poisson(lambda: prob.setup_multigrid(nu=1, omega=0.85))
    its_1, phi_1 = poisson(poly(1, weights=0.85))
    its_2, phi_2 = poisson(poly(2))
    assert len(prob.multigrid_levels) >= 3
    assert its_1 == its_v and np.allclose(phi_1, phi_v, rtol=1e-10, atol=1e-10 * np.abs(phi_v).max())
    assert its_2 < its_v and np.allclose(phi_2, phi_v, rtol=0, atol=1e-8 * np.abs(phi_v).max())
    prob.close()
    # as the alternative for hard systems (forced on by thresholds every solve exceeds)
    out = {}
    for hard in (None, 2):
        prob = streamer.device_problem(msh.coords, msh.cells)
        st = streamer.Stepper(prob)
        st.initialise()
        prob.setup_multigrid(nu=1, omega=0.85, hard_poly_degree=hard)
        from fedm_amd.device import chebyshev_weights
        prob.set_fieldsplit(chebyshev_weights(6), hard_weights=chebyshev_weights(6), switch_above=0.5, back_below=0.1)
        for _ in range(4):
            st.step()
        out[hard] = (st.newton_iterations, st.linear_iterations, prob.get_state())
        prob.close()
    assert out[None][0] == out[2][0] and out[2][1] <= out[None][1]
    scale = np.abs(out[None][2]).max(axis=0)
    assert (np.abs(out[None][2] - out[2][2]).max(axis=0) / scale).max() < 1e-6


@pytest.mark.parametrize("three_species,unstructured", [(False, False), (True, False), (True, True)])
def test_row_at_a_time_assembly_matches_the_unrolled_element(monkeypatch, three_species, unstructured):
    """F + J patches run through element_lean.hpp (one equation row at a time, rows as workgroup
    phases); FEDM_ASSEMBLY_LEAN=0 selects the unrolled element routine the oracle parity tests were
    written against.  Two implementations of the same tensors: residual and Jacobian must agree to
    rounding -- on the streamer model and on a model that exercises what the streamer does not
    (three species, a species drifting with a constant velocity, a reaction that is a loss for two
    species and a gain for the third, with a field-dependent rate) -- the latter also on a locally refined
    unstructured mesh (the <3 species, 256 threads> instantiations, turned cells)."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum, parse
    msh = streamer.refined_mesh(60e-6) if unstructured else streamer.mesh(24, 2.0)
    m = Mesh(msh.coords, msh.cells)
    tags = Marking_boundaries(m, streamer.BOUNDARIES)
    nv = m.coords.shape[0]
    rng = np.random.default_rng(3)
    x, y = m.coords[:, 0] / streamer.BOX, m.coords[:, 1] / streamer.BOX
    if three_species:
        mu = parse(streamer.MU_E)
        ionisation = parse(streamer.ALPHA) * mu * TermSum.field()
        model = Model(n_species=3, poisson=True,
                      eq_type=["diffusion-reaction", "drift-diffusion-reaction", "drift-diffusion-reaction"],
                      Z=[1.0, -1.0, -1.0], mu=[TermSum.const(0.0), mu, TermSum.const(0.0)],
                      D=[TermSum.const(5e-4), parse(streamer.D_E), TermSum.const(2e-3)],
                      reactions=[Reaction(ionisation * TermSum.const(1e-21), power=[1, 1, 0], net=[-1, -1, 1])],
                      drift_w=[None, None, (1.0e3, -2.0e3)], quadrature_degree=2)
        neq = 4
    else:
        model = streamer.model()
        neq = 3
    ddofs, dvals = streamer.dirichlet(m.coords)
    ddofs = (ddofs // 3) * neq + (neq - 1)
    U = np.zeros((nv, neq))
    U[:, 0] = 30.0 + 2.0 * np.sin(5 * x) * np.cos(3 * y)
    U[:, 1] = 28.0 + 3.0 * np.cos(4 * x) * np.sin(6 * y)
    if three_species:
        U[:, 2] = 25.0 + np.sin(3 * x + 2 * y)
    U[:, neq - 1] = streamer.U_W * y + 50.0 * np.sin(3 * x) * np.sin(np.pi * y)
    U0 = U + 0.01 * rng.standard_normal(U.shape)
    U1 = U + 0.02 * rng.standard_normal(U.shape)
    out = {}
    # one pass over the cells (where instantiated: the streamer family) with the model's structure compiled in ("3":
    # the benchmark deck has a precompiled signature) and read at run time ("3r") / row phases / unrolled
    for lean in ("3", "3r", "2", "0"):
        monkeypatch.setenv("FEDM_ASSEMBLY_LEAN", lean[0])
        monkeypatch.setenv("FEDM_LEAN3_SIG", "0" if lean == "3r" else "1")
        prob = DeviceProblem(m.coords, m.cells, model, facet_tags=tags if not three_species else None,
                             dirichlet_dofs=ddofs.astype(np.int32), dirichlet_vals=dvals)
        if not three_species and lean[0] == "3":
            assert prob.sizes()["model_structure"] == ("compiled in" if lean == "3" else "run time")
        prob.set_state(U, U0, U1)
        prob.set_step(5e-12, 4e-12)
        prob.jacobian()
        F, _ = prob.residual()
        prob.jacobian()
        out[lean] = (F, prob.jacobian_csr())
        prob.close()
    F0, J0 = out["0"]
    rowmax = abs(J0).max(axis=1).toarray().ravel()
    for lean in ("3", "3r", "2"):
        F1, J1 = out[lean]
        assert np.abs(F1 - F0).max() <= 1e-12 * np.abs(F0).max(), lean
        d = abs(J1 - J0)
        assert (d.max(axis=1).toarray().ravel() <= 1e-11 * rowmax + 1e-300).all(), lean


def test_persistent_assembly_kernels_give_the_same_system(monkeypatch):
    """assemble3.hip holds two launch forms of the one-pass assembly: a workgroup per patch (default) and the
    persistent, software-pipelined kernels whose workgroups take patch after patch (FEDM_LEAN3_PERSISTENT=1).  Same
    cell routine, different staging: residual and Jacobian must agree to the order of the LDS atomics -- also for
    the first full assembly (every plane written) and on a mesh whose patch count is not a multiple of the grid."""
    from fedm_amd.cases import streamer
    msh = streamer.refined_mesh(40e-6)
    nv = msh.coords.shape[0]
    rng = np.random.default_rng(5)
    x, y = msh.coords[:, 0] / streamer.BOX, msh.coords[:, 1] / streamer.BOX
    U = np.zeros((nv, 3))
    U[:, 0] = 30.0 + 2.0 * np.sin(5 * x) * np.cos(3 * y)
    U[:, 1] = 28.0 + 3.0 * np.cos(4 * x) * np.sin(6 * y)
    U[:, 2] = streamer.U_W * y + 50.0 * np.sin(3 * x) * np.sin(np.pi * y)
    U0 = U + 0.01 * rng.standard_normal(U.shape)
    U1 = U + 0.02 * rng.standard_normal(U.shape)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("FEDM_LEAN3_PERSISTENT", mode)
        prob = streamer.device_problem(msh.coords, msh.cells)
        assert prob.assembly_variant() == "lds-patches/one-pass"
        prob.set_state(U, U0, U1)
        prob.set_step(5e-12, 4e-12)
        prob.jacobian()                       # the first assembly writes every plane
        J_first = prob.jacobian_csr()
        prob.jacobian()                       # ... the later ones keep the constant ones
        F, _ = prob.residual()
        out[mode] = (F, J_first, prob.jacobian_csr())
        prob.close()
    F0, Ja0, Jb0 = out["0"]
    F1, Ja1, Jb1 = out["1"]
    assert np.abs(F1 - F0).max() <= 1e-13 * np.abs(F0).max()
    rowmax = abs(Jb0).max(axis=1).toarray().ravel()
    for A, B in ((Ja0, Ja1), (Jb0, Jb1), (Ja0, Jb0)):
        assert (abs(A - B).max(axis=1).toarray().ravel() <= 1e-12 * rowmax + 1e-300).all()


def test_state_checkpoint_on_the_device_repeats_the_steps(streamer_setup):
    """fedm_state_snapshot / fedm_state_restore (what bench.py repeats its timed window from): steps taken from
    a restored checkpoint reproduce the error log and the state of the steps taken after the checkpoint was made."""
    from fedm_amd.cases import streamer
    msh = streamer.mesh(48, 4.0)
    st = streamer.Stepper(streamer.device_problem(msh.coords, msh.cells))
    st.initialise()
    for _ in range(3):
        st.step()
    snap = st.snapshot()
    first = []
    for _ in range(4):
        st.step()
        first.append((st.t, st.dt.time_step, tuple(st.max_error)))
    U_first = st.prob.get_state()
    st.restore(snap)
    assert st.steps == 3
    again = []
    for _ in range(4):
        st.step()
        again.append((st.t, st.dt.time_step, tuple(st.max_error)))
    U_again = st.prob.get_state()
    for a, b in zip(first, again):
        assert a[0] == b[0] and a[1] == b[1] and np.allclose(a[2], b[2], rtol=1e-6)
    # (the Krylov path of a repeated solve may differ -- launch-ahead hints -- within the solver tolerances)
    assert (np.abs(U_again - U_first).max(axis=0) / np.abs(U_first).max(axis=0)).max() < 1e-7
    st.prob.close()


def test_preconditioner_side_left_and_right_agree():
    """The Newton systems are solved by flexible GMRES with the field split on the right (true
    residual norm) or, selectable, on the left (preconditioned residual norm).  Both solve
    J delta = -F to ksp_rtol: same Newton iteration counts, same trajectory within the solver
    tolerances, and the right variant needs no more Krylov steps."""
    from fedm_amd.cases import streamer
    msh = streamer.mesh(48, 4.0)
    out = {}
    for side in ("left", "right"):
        prob = streamer.device_problem(msh.coords, msh.cells)
        prob.set_preconditioner_side(side)
        st = streamer.Stepper(prob)
        st.initialise()
        for _ in range(4):
            st.step()
        out[side] = (st.newton_iterations, st.linear_iterations, prob.get_state(), st.log_rows())
        prob.close()
    assert out["left"][0] == out["right"][0]
    assert out["right"][1] <= out["left"][1]
    scale = np.abs(out["left"][2]).max(axis=0)
    assert (np.abs(out["left"][2] - out["right"][2]).max(axis=0) / scale).max() < 1e-6
    assert np.allclose(np.array(out["left"][3]), np.array(out["right"][3]), rtol=1e-4)
    with pytest.raises(KeyError):
        prob.set_preconditioner_side("middle")


def test_fieldsplit_order_lower_and_upper_solve_the_same_systems():
    """Order of the block-triangular split on the right: species first (default) or potential first
    (opt-in, include/fedm_hip.h).  Both solve J delta = -F to ksp_rtol in the residual norm: same
    Newton counts, same trajectory within the solver tolerances early in a run (where the potential
    block is easy; what the orders do late is recorded by tools/fs_order_accuracy.py)."""
    from fedm_amd.cases import streamer
    msh = streamer.mesh(48, 4.0)
    out = {}
    for order in ("lower", "upper"):
        prob = streamer.device_problem(msh.coords, msh.cells)
        st = streamer.Stepper(prob)
        st.initialise()
        prob.set_fieldsplit_order(order)
        for _ in range(4):
            st.step()
        out[order] = (st.newton_iterations, st.linear_iterations, prob.get_state(), st.log_rows())
        prob.close()
    assert out["lower"][0] == out["upper"][0]
    assert out["upper"][1] <= out["lower"][1] + 2
    scale = np.abs(out["lower"][2]).max(axis=0)
    assert (np.abs(out["lower"][2] - out["upper"][2]).max(axis=0) / scale).max() < 1e-5
    assert np.allclose(np.array(out["lower"][3]), np.array(out["upper"][3]), rtol=1e-3)
    with pytest.raises(KeyError):
        prob.set_fieldsplit_order("diagonal")


def test_coupling_product_inside_the_last_sweep_changes_the_preconditioner_only(monkeypatch):
    """The field split's coupling product b_phi -= J_phi,u z_u is formed inside the last species sweep
    from the iterate before that sweep (default) or by its own kernel from the final iterate
    (FEDM_FS_LAGGED_COUPLING=0).  Two preconditioners for the same systems: same Newton counts, Krylov
    counts within a step or two, same trajectory within the solver tolerances."""
    from fedm_amd.cases import streamer
    msh = streamer.mesh(64, 4.0)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("FEDM_FS_LAGGED_COUPLING", flag)
        prob = streamer.device_problem(msh.coords, msh.cells)
        st = streamer.Stepper(prob)
        st.initialise()
        for _ in range(6):
            st.step()
        out[flag] = (st.newton_iterations, st.linear_iterations, prob.get_state(), st.log_rows())
        prob.close()
    assert out["1"][0] == out["0"][0]
    assert abs(out["1"][1] - out["0"][1]) <= 3
    scale = np.abs(out["0"][2]).max(axis=0)
    assert (np.abs(out["1"][2] - out["0"][2]).max(axis=0) / scale).max() < 1e-6
    assert np.allclose(np.array(out["1"][3]), np.array(out["0"][3]), rtol=1e-3)


def test_graft_entry_smoke():
    """The driver's smoke() entry point (one small streamer solve checked against the oracle)."""
    import __graft_entry__ as entry
    entry.smoke()


def test_numerical_failures_raise_and_adaptive_solver_recovers(tmp_path):
    """Error behaviour of the boundary: positive return codes of the C ABI become
    RuntimeError, which adaptive_solver's catch-all (fedm/functions.py:1080-1127) answers by
    halving the step and repeating; a step whose error exceeds ttol is repeated with
    dt * 0.5 * ttol / error (:1090-1101)."""
    from fedm_amd.cases import streamer
    msh = streamer.mesh(32, 4.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    U, _ = streamer.initialise(prob)
    # (1) Newton cannot converge in one iteration -> FEDM_DIVERGED_MAX_IT -> RuntimeError
    prob.set_step(5e-12, 1e30)
    with pytest.raises(RuntimeError, match="maximum"):
        prob.newton_solve(rtol=1e-12, max_it=1)
    # (2) NaN in the state -> FEDM_DIVERGED_NAN -> RuntimeError
    bad = U.copy()
    bad[5, 1] = np.nan
    prob.set_state(bad, U, U)
    with pytest.raises(RuntimeError, match="NaN"):
        prob.newton_solve(rtol=1e-4, max_it=20)
    # (3) the time loop recovers from both kinds of rejection
    prob.set_state(U, U, U)
    st = streamer.Stepper(prob, dt_init=4e-10, dt_max=4e-10, error_file=tmp_path / "relative error.log")
    st.step()
    rows = np.loadtxt(tmp_path / "relative error.log", ndmin=2)
    assert st.dt_old.time_step < 4e-10                 # the accepted step is shorter than the first try
    assert rows[-1, 0] < st.ttol                       # last logged attempt was accepted
    assert len(rows) >= 2 or st.dt_old.time_step < 4e-10
    assert np.all(np.isfinite(prob.get_state()))
    prob.close()


def test_bad_descriptors_are_hard_errors():
    """Negative return codes (bad descriptor) raise with the library's message."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem
    msh = streamer.mesh(8, 1.0)
    cells = msh.cells.copy()
    cells[3, 1] = msh.coords.shape[0] + 7              # vertex index out of range
    with pytest.raises(ValueError, match="out of range"):
        DeviceProblem(msh.coords, cells, streamer.model())
    # the C ABI checks on its own as well (a caller that binds the library directly)
    from fedm_amd import _lib
    import ctypes as C
    lib = _lib.load()
    prob = streamer.device_problem(msh.coords, msh.cells)
    rc = lib.fedm_set_fieldsplit(prob._h, 0, None)
    assert rc < 0 and b"sweeps" in lib.fedm_last_error()
    assert lib.fedm_set_fieldsplit_order(prob._h, 2) < 0 and b"order" in lib.fedm_last_error()
    # a polynomial-smoother hierarchy needs a degree, weights and at least two levels
    assert lib.fedm_amg_setup_poly(prob._h, 1, None, None, None, None, 0, None, 0) < 0
    assert b"polynomial" in lib.fedm_last_error()
    kept, zero = prob.plane_masks()
    assert zero == 0b1000 and kept & (1 << 8)     # d(electron row)/d(ion density); potential-potential
    prob.close()


def test_streamer_parity_at_128_squared_against_both_cpu_statements():
    """The streamer's |E|-dependent coefficients, alpha(E) source and Neumann drift flux have no
    reference-held vector behind them (mesh.xml and the field goldens are missing blobs upstream),
    so the HIP path is held against TWO independent CPU statements of the same forms on a 128 x 128
    graded mesh (16 641 vertices, 130 patches: several full LDS patches in every direction, unlike
    the 441-vertex meshes above): the vectorised numpy oracle (direct quadrature, oracle/forms.py)
    and the C/OpenMP element loop (oracle/cpu/fedm_cpu.c), for a developed-looking state with
    steep density gradients and a non-uniform field."""
    from oracle import cpu_backend as cb
    from oracle import streamer as ost
    from oracle.mesh import graded_axis, rectangle_right
    from fedm_amd.cases import streamer
    n = 128
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, n, n, xs=graded_axis(ost.BOX, n, 4.0))
    omodel = ost.build(mesh)
    r, z = mesh.coords[:, 0], mesh.coords[:, 1]
    rng = np.random.default_rng(11)
    U = np.zeros((mesh.nv, 3))
    head = np.exp(-(r ** 2 + (z - 0.008) ** 2) / (0.6e-3) ** 2)
    U[:, 0] = np.log(1e13 + 4e19 * head) + 0.02 * rng.standard_normal(mesh.nv)
    U[:, 1] = np.log(1e13 + 3e19 * head) + 0.02 * rng.standard_normal(mesh.nv)
    U[:, 2] = ost.U_W * z / ost.BOX * (1.0 + 0.3 * head) + 5.0 * rng.standard_normal(mesh.nv)
    Uo = U + 0.01 * rng.standard_normal(U.shape)
    Uo1 = U + 0.02 * rng.standard_normal(U.shape)
    dt, dt_old = 5e-12, 4.977e-12
    F_np, J_np = omodel.residual_jacobian(U, Uo, Uo1, dt, dt_old)
    cprob = cb.CpuProblem(omodel)
    cprob.set_state(U, Uo, Uo1)
    F_c, J_c = cprob.residual_jacobian(dt, dt_old)
    cprob.close()
    prob = streamer.device_problem(mesh.coords, mesh.cells)
    prob.set_state(U, Uo, Uo1)
    prob.set_step(dt, dt_old)
    F_gpu, _ = prob.residual()          # residual-only kernel
    prob.jacobian()                     # F + J kernel
    J_gpu = prob.jacobian_csr()
    prob.close()
    scale = np.abs(F_np).reshape(-1, 3).max(axis=0)
    for F_ref in (F_np, F_c):
        assert (np.abs(F_gpu - F_ref).reshape(-1, 3) / scale).max() < 1e-11
    assert _rel_rows(J_gpu, J_np) < 1e-10
    assert _rel_rows(J_gpu, J_c) < 1e-10


@pytest.mark.parametrize("n", [128, 192])
def test_streamer_error_log_has_the_structure_of_the_reference_log(n, golden_dir):
    """The one streamer artefact the reference still holds is its 21-row error log
    (tests/integrated_tests/streamer_discharge/20220707_results/relative error.log): accepted
    steps only, dt = dt_max = 5e-12 throughout (one step shortened to 4.977e-12 by the controller
    because the logged change, 6.7e-4, sits just under ttol = 1e-3), the per-step relative change
    of ln n_e falling by 6-8 parts in 1e4 from step to step.  The value of that change is the
    ratio of two vector norms over the vertices, i.e. it depends on how the (missing) reference mesh
    distributes its vertices and cannot be reproduced on another mesh; what does carry over is
    checked on two of our meshes: no rejected step up to 1e-10 s, every dt the controller proposes
    stays at dt_max once the change is far below ttol, the change decays monotonically by about
    one part in a thousand per step like the reference's (0.7e-3 there, 1.4e-3 on these meshes: the
    same order, the norm's vertex weighting again), and it is mesh-converged between the two
    resolutions."""
    import json
    from fedm_amd.cases import streamer
    ref = np.array(json.loads((golden_dir / "error_logs.json").read_text())["streamer_discharge"])
    assert ref.shape == (21, 3) and np.all(ref[:, 0] < 1e-3)              # all accepted
    ref_decay = ref[5:20, 0] / ref[4:19, 0]                                # constant-dt stretch
    msh = streamer.mesh(n, 4.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    out = streamer.run(prob, T_final=1e-10)
    prob.close()
    log = np.array(out["log"])
    assert out["steps"] == len(log) == 20                                  # no rejection, no retry
    assert np.all(log[:, 2] == 5e-12) and log[0, 1] == 1e30 and np.all(log[1:, 1] == 5e-12)
    assert out["t"] == pytest.approx(1e-10, rel=1e-9)
    decay = log[5:, 0] / log[4:-1, 0]
    assert np.all(decay < 1.0) and np.all(np.diff(decay) < 0)             # monotone, slowly steepening: as in the reference
    assert np.all(np.diff(ref_decay) < 0)
    assert 0.3 < (1.0 - decay.mean()) / (1.0 - ref_decay.mean()) < 3.0
    _CHANGE[n] = log[:, 0]
    if len(_CHANGE) == 2:                                                  # mesh convergence of the logged quantity
        a, b = _CHANGE[128], _CHANGE[192]
        assert np.abs(a / b - (a / b).mean()).max() < 2e-3


_CHANGE = {}


def test_non_logarithmic_representation_matches_the_oracle():
    """`weak_form_balance_equation(..., log_representation=False)` / `Flux(...,
    logarithm_representation=False)` (fedm/functions.py:219-237, 350-368): the unknowns are the
    densities themselves.  PARITY UNPINNED (no reference example, test or golden uses the form):
    the device element (generic `Element<..., LIN = true>`, both assembly variants) against the
    oracle's statement of the same integrals, whose Jacobian is checked against finite differences
    in tests/test_oracle_linear.py; and a Newton solve against the oracle's."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_oracle_linear import _model, _state
    from oracle import streamer as ost
    from oracle.mesh import graded_axis, rectangle_right
    from oracle.newton import newton_solve
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum, parse
    n = 20
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, n, n, xs=graded_axis(ost.BOX, n, 3.0))
    omodel = _model(mesh, log=False)
    lnn, phi = _state(mesh, seed=9)
    U = np.column_stack([np.exp(lnn), phi])
    Uo, Uo1 = U * (1.0 + 1e-3), U * (1.0 - 2e-3)
    dt, dt_old = 5e-12, 4e-12
    mu = parse(streamer.MU_E)
    rate = parse(streamer.ALPHA) * mu * TermSum.field()
    model = Model(n_species=2, poisson=True, eq_type=["reaction", "drift-diffusion-reaction"], Z=[1.0, -1.0],
                  mu=[TermSum.const(0.0), mu], D=[TermSum.const(0.0), parse(streamer.D_E)],
                  reactions=[Reaction(rate, power=[0, 1], net=[1, 1])], bc_kind=streamer.BC_TYPE,
                  quadrature_degree=2, log_representation=False)
    m = Mesh(mesh.coords, mesh.cells)
    tags = Marking_boundaries(m, streamer.BOUNDARIES)
    ddofs, dvals = streamer.dirichlet(m.coords)
    F_cpu, J_cpu = omodel.residual_jacobian(U, Uo, Uo1, dt, dt_old)
    scale = np.abs(F_cpu).reshape(-1, 3).max(axis=0)
    for kind in ("patch", "colour"):                  # LDS patches, global colouring
        prob = DeviceProblem(m.coords, m.cells, model, facet_tags=tags, dirichlet_dofs=ddofs, dirichlet_vals=dvals)
        prob.set_assembly(kind)
        prob.set_state(U, Uo, Uo1)
        prob.set_step(dt, dt_old)
        F_gpu, _ = prob.residual()
        assert (np.abs(F_gpu - F_cpu).reshape(-1, 3) / scale).max() < 1e-11
        prob.jacobian()
        assert _rel_rows(prob.jacobian_csr(), J_cpu) < 1e-10
        if kind == "patch":
            # one Newton solve from the old state (point-block Jacobi GMRES: no hierarchy installed)
            prob.set_state(Uo, Uo, Uo1)
            its, _ = prob.newton_solve(rtol=1e-9, max_it=20, ksp_rtol=1e-12, ksp_max_it=5000)
            U_gpu = prob.get_state()
            U_cpu = Uo.copy()
            its_cpu, _ = newton_solve(omodel, U_cpu, Uo, Uo1, dt, dt_old, 1e-9, 20)
            assert its == its_cpu
            assert (np.abs(U_gpu - U_cpu).max(axis=0) / np.abs(U_cpu).max(axis=0)).max() < 1e-8
        prob.close()


def test_measured_choice_of_the_hard_regime_set_is_the_same_solve(monkeypatch):
    """In the hard regime (here forced: thresholds below any Krylov count) the library times its own Newton
    solves and uses the faster of the two preconditioner sets, probing the other now and then; round 2's rule
    (FEDM_FS_POLICY=counts) always takes the alternative set there.  Different preconditioners, the same
    systems solved to the same tolerance: same accepted steps, Newton counts and -- within the Newton
    tolerance -- states."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    msh = streamer.mesh(64, 4.0)
    out = {}
    for policy in ("measured", "counts"):
        if policy == "counts":
            monkeypatch.setenv("FEDM_FS_POLICY", "counts")
        prob = streamer.device_problem(msh.coords, msh.cells)
        st = streamer.Stepper(prob)
        st.initialise()
        prob.set_fieldsplit(chebyshev_weights(6), hard_weights=chebyshev_weights(4), switch_above=1.0, back_below=0.5)
        for _ in range(24):
            st.step()
        out[policy] = (prob.get_state(), st.newton_iterations, st.linear_iterations, np.array(st.log_rows()))
        prob.close()
    (Um, nm, lm, logm), (Uc, nc, lc, logc) = out["measured"], out["counts"]
    assert nm == nc and logm.shape == logc.shape == (24, 3)
    assert np.allclose(logm, logc, rtol=1e-4)
    assert np.allclose(Um, Uc, rtol=1e-5, atol=1e-5)
    assert 0.5 * lc <= lm <= 2.0 * lc


def test_species_planes_formed_by_the_assembly_equal_the_separate_pass(monkeypatch):
    """With FEDM_PLANES_FUSED=1 (opt-in: it did not pay in the step) the one-pass kernel forms the
    field split's planes (Duu^-1, the half-precision species planes, the single-precision coupling plane) from its
    LDS accumulators while it streams the Jacobian out, from the second Jacobian assembly of a run on, and `species_planes_rows_kernel` redoes the rows changed behind it (boundary facets,
    Dirichlet values, padding): together they must leave what the separate pass over the finished matrix leaves.
    Also: the run itself is the one FEDM_PLANES_FUSED=0 gives."""
    from fedm_amd.cases import streamer
    logs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("FEDM_PLANES_FUSED", fused)
        for msh in (streamer.mesh(48, 4.0), streamer.refined_mesh(40e-6)):
            st = streamer.Stepper(streamer.device_problem(msh.coords, msh.cells))
            st.initialise()
            used = []
            for _ in range(3):
                st.step()
                d_inv, d_s16, d_cpl, was_fused = st.prob.species_planes_check()
                used.append(was_fused)
                assert d_inv <= 1e-14 and d_cpl == 0.0, (fused, d_inv, d_cpl)
                assert d_s16 <= 2e-3, (fused, d_s16)       # (entries of Duu^-1 J_uu are O(1): half an ulp of fp16)
            assert all(used) == (fused == "1") and any(used) == (fused == "1")
            logs.setdefault(msh.coords.shape[0], {})[fused] = (st.newton_iterations, st.linear_iterations,
                                                               st.prob.get_state())
            st.prob.close()
    for nv, by in logs.items():
        assert by["1"][:2] == by["0"][:2], (nv, by["1"][:2], by["0"][:2])
        assert np.abs(by["1"][2] - by["0"][2]).max() <= 1e-9 * np.abs(by["0"][2]).max()


def test_one_pass_assembly_of_models_with_another_structure_than_the_benchmark_deck(monkeypatch):
    """The one-pass kernels are instantiated with the benchmark deck's STRUCTURE compiled in (which equation a species
    has, the reaction's powers, the terms of the coefficient functions and the atoms they multiply) and with the
    structure read from the plan at run time.  Models of the same family with other structures -- constant diffusion,
    a mobility that shares its power atom with the diffusion, an ionisation coefficient without the E^-3 term -- must
    take the run-time kernels; the deck's terms in another order or with other exponents the compiled ones (the plan
    is canonical, the numbers stay run-time data); all give the system of the unrolled element routine."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum, parse
    msh = streamer.mesh(24, 2.0)
    m = Mesh(msh.coords, msh.cells)
    tags = Marking_boundaries(m, streamer.BOUNDARIES)
    nv = m.coords.shape[0]
    rng = np.random.default_rng(8)
    x, y = m.coords[:, 0] / streamer.BOX, m.coords[:, 1] / streamer.BOX
    ddofs, dvals = streamer.dirichlet(m.coords)
    U = np.zeros((nv, 3))
    U[:, 0] = 30.0 + 2.0 * np.sin(5 * x) * np.cos(3 * y)
    U[:, 1] = 28.0 + 3.0 * np.cos(4 * x) * np.sin(6 * y)
    U[:, 2] = streamer.U_W * y + 50.0 * np.sin(3 * x) * np.sin(np.pi * y)
    U0 = U + 0.01 * rng.standard_normal(U.shape)
    U1 = U + 0.02 * rng.standard_normal(U.shape)

    def build(mu_e, D_e, alpha):
        mu = parse(mu_e)
        return Model(n_species=2, poisson=True, eq_type=["reaction", "drift-diffusion-reaction"], Z=[1.0, -1.0],
                     mu=[TermSum.const(0.0), mu], D=[TermSum.const(0.0), parse(D_e)],
                     reactions=[Reaction(parse(alpha) * mu * TermSum.field(), power=[0, 1], net=[1, 1])],
                     bc_kind=streamer.BC_TYPE, quadrature_degree=2)
    cases = {
        "the deck": (streamer.MU_E, streamer.D_E, streamer.ALPHA, "compiled in"),
        "the deck, alpha's terms in another order": (streamer.MU_E, streamer.D_E,
                                                     "-340.75 + (4.3666e26*E_m**(-3) + 1.1944e6)*exp(-2.73e7/E_m)", "compiled in"),
        "constant diffusion": (streamer.MU_E, "0.18", streamer.ALPHA, "run time"),
        # (the same structure with other NUMBERS is the compiled one: two power atoms, the same terms)
        "mobility with another exponent": ("2.3987*E_m**(-0.31)", streamer.D_E, streamer.ALPHA, "compiled in"),
        "mobility and diffusion sharing their power atom": ("2.3987*E_m**(-0.78)", streamer.D_E, streamer.ALPHA, "run time"),
        "alpha without the E^-3 term": (streamer.MU_E, streamer.D_E, "1.1944e6*exp(-2.73e7/E_m) - 340.75", "run time"),
    }
    for name, (mu_e, D_e, alpha, structure) in cases.items():
        model = build(mu_e, D_e, alpha)
        out = {}
        for lean in ("3", "0"):
            monkeypatch.setenv("FEDM_ASSEMBLY_LEAN", lean)
            prob = DeviceProblem(m.coords, m.cells, model, facet_tags=tags, dirichlet_dofs=ddofs.astype(np.int32),
                                 dirichlet_vals=dvals)
            if lean == "3":
                sz = prob.sizes()
                assert sz["assembly_variant"] == "lds-patches/one-pass", name
                assert sz["model_structure"] == structure, (name, sz["model_structure"])
            prob.set_state(U, U0, U1)
            prob.set_step(5e-12, 4e-12)
            prob.jacobian()
            F, _ = prob.residual()
            prob.jacobian()
            out[lean] = (F, prob.jacobian_csr())
            prob.close()
        F0, J0 = out["0"]
        F1, J1 = out["3"]
        rowmax = abs(J0).max(axis=1).toarray().ravel()
        assert np.abs(F1 - F0).max() <= 1e-12 * np.abs(F0).max(), name
        assert (abs(J1 - J0).max(axis=1).toarray().ravel() <= 1e-11 * rowmax + 1e-300).all(), name


@pytest.mark.parametrize("lean", ["2", "0"])
def test_four_species_and_poisson_against_the_oracle(monkeypatch, lean):
    """The largest model `fedm_model_desc` holds (FEDM_MAX_SPECIES = 4 + Poisson, five equations): a metastable that only
    diffuses, an ion that drifts, a negative ion drifting with a prescribed velocity, electrons with field-dependent
    coefficients; three reactions with field-dependent, constant and quadratic rates.  Residual, Jacobian, product and
    a Newton step of the device path (row-phase kernels / unrolled element routine) against the numpy oracle
    (oracle/forms.py restates fedm/functions.py:240-401 for any number of species)."""
    from fedm_amd.cases import streamer
    from lfa_models import four_species_problem
    monkeypatch.setenv("FEDM_ASSEMBLY_LEAN", lean)
    m, prob, om, ddofs, dvals = four_species_problem()
    nv = m.coords.shape[0]
    assert prob.assembly_variant() == ("lds-patches" if lean == "2" else "lds-patches/unrolled")
    rng = np.random.default_rng(4)
    x, y = m.coords[:, 0] / streamer.BOX, m.coords[:, 1] / streamer.BOX
    U = np.zeros((nv, 5))
    U[:, 0] = 27.0 + np.sin(4 * x) * np.cos(2 * y)
    U[:, 1] = 30.0 + 2.0 * np.sin(5 * x) * np.cos(3 * y)
    U[:, 2] = 25.0 + np.sin(3 * x + 2 * y)
    U[:, 3] = 29.0 + 2.0 * np.cos(4 * x) * np.sin(6 * y)
    U[:, 4] = streamer.U_W * y + 50.0 * np.sin(3 * x) * np.sin(np.pi * y)
    U.ravel()[ddofs] = dvals
    Uo = U + 0.01 * rng.standard_normal(U.shape)
    Uo1 = U + 0.02 * rng.standard_normal(U.shape)
    dt, dt_old = 5e-12, 4e-12
    prob.set_state(U, Uo, Uo1)
    prob.set_step(dt, dt_old)
    F_gpu, fnorm = prob.residual()
    F_cpu, J_cpu = om.residual_jacobian(U, Uo, Uo1, dt, dt_old)
    scale = np.abs(F_cpu).reshape(-1, 5).max(axis=0)
    assert (np.abs(F_gpu - F_cpu).reshape(-1, 5) / scale).max() < 1e-11
    assert fnorm == pytest.approx(np.linalg.norm(F_cpu), rel=1e-11)
    prob.jacobian()
    assert prob.launched_assembly()["jacobian"]["variant"] == ("lds-patches" if lean == "2" else "lds-patches/unrolled")
    J_gpu = prob.jacobian_csr()
    assert _rel_rows(J_gpu, J_cpu) < 1e-10
    xv = rng.normal(size=prob.n)
    yv, yc = prob.spmv(xv), J_cpu @ xv
    assert np.abs(yv - yc).max() / np.abs(yc).max() < 1e-11
    # a Newton solve of one time step (point-block Jacobi GMRES here; then with the field split: species polynomial +
    # multigrid on the potential block) against the oracle's Newton with direct solves
    from oracle.newton import newton_solve
    from fedm_amd.device import chebyshev_weights
    U_cpu = Uo.copy()
    its_cpu, _ = newton_solve(om, U_cpu, Uo, Uo1, dt, dt_old, 1e-8, 25)
    for split in (False, True):
        prob.set_state(Uo, Uo, Uo1)
        prob.set_step(dt, dt_old)
        if split:
            prob.setup_multigrid(**streamer.MULTIGRID)
            prob.set_fieldsplit(chebyshev_weights(6))
        its, _ = prob.newton_solve(rtol=1e-8, max_it=25, ksp_rtol=1e-10, ksp_max_it=2000)
        assert its == its_cpu, (split, its, its_cpu)
        d = np.abs(prob.get_state() - U_cpu).max(axis=0) / np.abs(U_cpu).max(axis=0)
        assert d.max() < 1e-8, (split, d)
    prob.close()
