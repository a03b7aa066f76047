"""The segregated (uncoupled) time step on the device -- ``fedm_poisson_update`` + ``fedm_newton_solve_species`` --
against the float64 restatement (tests/segregated_reference.py) and the oracle's blocks.

Contexts: ``streamer.mesh(48, 4.0)`` in the states of test_gpu_krylov._streamer48 ("init": the early streamer; "head": a
developed head), one of tests/limit_meshes.py's meshes beyond 256 cells a patch, the four-species model (which takes
the fallback assembly) and the 17 k-vertex unstructured mesh.

Bounds set in advance (none comes from what the device gives):
  F species rows against the oracle <= 1e-11, J_uu <= 1e-10 (relative to the largest entry), F of the
  potential rows exactly 0; the true species residual of a linear solve <= FIXED[ksp_rtol] * tol (test_gpu_krylov.py);
  state against the restatement <= 1e-9 with both solved to 1e-8 / 1e-10; poisson_update within 1e-9 of the direct
  solve (the bound test_streamer_poisson_solve has for fedm_poisson_solve).

Five steps at fixed dt = 5 ps against five restated steps: measured on the MI355X and bounded at 10x the measured value
(the convention of DRIFT_BOUND in test_gpu_krylov.py).
"""
import numpy as np
import pytest

import segregated_reference as sr

pytestmark = pytest.mark.gpu

MAX_IT, NAN = 1, 2            # FEDM_DIVERGED_MAX_IT, FEDM_DIVERGED_NAN
FIXED = {1e-5: 2.0, 1e-10: 10.0}      # test_gpu_krylov.FIXED
STATE_BOUND = 1e-9
# Five segregated steps (dt 5 ps, species rtol 1e-10 / ksp_rtol 1e-12, Poisson 1e-12) against five restated steps, worst
# component, relative to the component's largest value.  MI355X, 2026-10-17:
#   state    measured
#   init     1.8e-15 (ions 1.8e-15, electrons 1.6e-15, potential 1.2e-15)
MEASURED = {"init": 1.8e-15}
FIVE_STEP_BOUND = {k: 10.0 * v for k, v in MEASURED.items()}


# ---- contexts ------------------------------------------------------------------------------------------------------
def _head_arrays(coords, nv):
    """test_gpu_preconditioner._head_state's arrays (same generator, same order of draws)."""
    from fedm_amd.cases import streamer
    r, z = coords[:, 0], coords[:, 1]
    rng = np.random.default_rng(5)
    head = np.exp(-(r ** 2 + (z - 0.008) ** 2) / (0.6e-3) ** 2)
    U = np.zeros((nv, 3))
    U[:, 0] = np.log(1e13 + 4e19 * head) + 0.02 * rng.standard_normal(nv)
    U[:, 1] = np.log(1e13 + 3e19 * head) + 0.02 * rng.standard_normal(nv)
    U[:, 2] = streamer.U_W * z / streamer.BOX * (1.0 + 0.3 * head)
    return U, U + 0.01 * rng.standard_normal(U.shape), U.copy(), 5e-12, 4e-12


def _oracle(coords, cells):
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    return ost.build(OMesh(coords, cells))


def _context(state, mesh="48", multigrid=True, weights=6, perturb=False):
    """(device problem, oracle model, (U, Uold, Uold1, dt, dt_old)) with the state set on the device.  perturb: the
    new state moved away from the old one (with u == u_old the BDF term of F is cancellation noise and a relative
    bound on F means nothing: the assembly checks compare at a perturbed state)."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    if mesh == "48":
        msh = streamer.mesh(48, 4.0)
        coords, cells = msh.coords, msh.cells
        prob = streamer.device_problem(coords, cells)
    elif mesh == "refined":
        msh = streamer.refined_mesh(30e-6)
        coords, cells = msh.coords, msh.cells
        prob = streamer.device_problem(coords, cells)
    else:
        import limit_meshes
        coords, cells = limit_meshes.build(mesh)
        prob = limit_meshes.device_problem(coords, cells)
    om = _oracle(coords, cells)
    if state == "init":
        from oracle import streamer as ost
        U0 = ost.initial_state(om)
        U1 = U0.copy()
        if perturb:
            x, y = coords[:, 0] / ost.BOX, coords[:, 1] / ost.BOX
            U1[:, 0] += 0.05 * np.sin(7.0 * x) * np.cos(5.0 * y)
            U1[:, 1] += 0.05 * np.cos(3.0 * x) * np.sin(4.0 * y)
        st = (U1, U0.copy(), U0.copy(), 5e-12, 1e30)
    else:
        st = _head_arrays(prob.coords, prob.nv)
    prob.set_state(st[0], st[1], st[2])
    prob.set_step(st[3], st[4])
    if multigrid:
        prob.setup_multigrid(nu=1, omega=0.85, max_coarse=40 if prob.nv < 5000 else 2000)
    if weights:
        prob.set_fieldsplit(chebyshev_weights(weights))
    return prob, om, st


def _species_assembly(prob):
    """The species F + J assembly alone, as a species Newton iteration runs it."""
    prob.species_assembly(jacobian=True)
    return prob.residual_vector(), prob.jacobian_csr()


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _check_assembly(prob, om, st, one_pass):
    U, Uo, Uo1, dt, dto = st
    n_eq = U.shape[1]
    iu, ip = sr.block_indices(U.size, n_eq)
    before = prob.segregated_stats()
    F, J = _species_assembly(prob)
    after = prob.segregated_stats()
    Fo, Jo = om.residual_jacobian(U, Uo, Uo1, dt, dto)
    eF = _rel(F[iu], Fo[iu])
    eJ = abs(sr.species_block(J, n_eq) - sr.species_block(Jo, n_eq)).max() / abs(sr.species_block(Jo, n_eq)).max()
    ran = {k: after[k] - before[k] for k in ("one_pass_assemblies", "fallback_assemblies")}
    print(f"[segregated] assembly: F_u {eF:.2e} J_uu {eJ:.2e} F_phi max {np.abs(F[ip]).max():.1e} {ran} "
          f"launched {prob.launched_assembly()}", flush=True)
    assert np.all(F[ip] == 0.0)
    assert eF <= 1e-11 and eJ <= 1e-10
    assert ran == ({"one_pass_assemblies": 1, "fallback_assemblies": 0} if one_pass
                   else {"one_pass_assemblies": 0, "fallback_assemblies": 1})
    return J


# ---- assembly ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["init", "head"])
def test_species_assembly_one_pass(state):
    prob, om, st = _context(state, multigrid=False, weights=0, perturb=True)
    _check_assembly(prob, om, st, one_pass=True)


def test_species_assembly_keeps_the_other_planes_and_the_first_coupled_jacobian_writes_all():
    prob, om, st = _context("head", multigrid=False, weights=0)
    U, Uo, Uo1, dt, dto = st
    n_eq = 3
    iu, ip = sr.block_indices(U.size, n_eq)
    # species-only assemblies first: the first coupled Jacobian of the context must still write every plane
    _check_assembly(prob, om, st, one_pass=True)
    prob.jacobian()
    Jo = om.residual_jacobian(U, Uo, Uo1, dt, dto)[1]
    Jc = prob.jacobian_csr()
    assert abs(Jc - Jo).max() / abs(Jo).max() <= 1e-10
    # a species-only assembly at ANOTHER state rewrites J_uu and leaves the potential row and column bit-identical
    U2 = U.copy()
    U2[:, :2] += 0.01 * np.sin(np.arange(prob.nv))[:, None]
    prob.set_state(U2, Uo, Uo1)
    J2 = _check_assembly(prob, om, (U2, Uo, Uo1, dt, dto), one_pass=True).tocsr()
    Jc = Jc.tocsr()
    for rows, cols in ((ip, np.arange(U.size)), (iu, ip)):
        a, b = Jc[rows][:, cols], J2[rows][:, cols]
        assert (a != b).nnz == 0
    # ... and the kept potential-potential plane is still right for the next coupled assembly
    prob.jacobian()
    Jo2 = om.residual_jacobian(U2, Uo, Uo1, dt, dto)[1]
    assert abs(prob.jacobian_csr() - Jo2).max() / abs(Jo2).max() <= 1e-10


def test_species_assembly_beyond_256_cells_a_patch():
    prob, om, st = _context("init", mesh="cells384", multigrid=False, weights=0, perturb=True)
    assert prob.sizes()["max_patch_cells"] > 256
    _check_assembly(prob, om, st, one_pass=True)


def test_species_assembly_unstructured_17k():
    prob, om, st = _context("head", mesh="refined", multigrid=False, weights=0)
    assert prob.nv > 15000
    _check_assembly(prob, om, st, one_pass=True)


def test_four_species_takes_the_fallback_and_solves():
    from lfa_models import four_species_problem
    from fedm_amd.cases import streamer
    m, prob, om, ddofs, dvals = four_species_problem()
    x, y = m.coords[:, 0] / streamer.BOX, m.coords[:, 1] / streamer.BOX
    rng = np.random.default_rng(4)
    U = np.zeros((prob.nv, 5))
    U[:, 0] = 27.0 + np.sin(4 * x) * np.cos(2 * y)
    U[:, 1] = 30.0 + 2.0 * np.sin(5 * x) * np.cos(3 * y)
    U[:, 2] = 25.0 + np.sin(3 * x + 2 * y)
    U[:, 3] = 29.0 + 2.0 * np.cos(4 * x) * np.sin(6 * y)
    U[:, 4] = streamer.U_W * y + 50.0 * np.sin(3 * x) * np.sin(np.pi * y)
    U.ravel()[ddofs] = dvals
    Uo, Uo1 = U + 0.01 * rng.standard_normal(U.shape), U + 0.02 * rng.standard_normal(U.shape)
    prob.set_state(U, Uo, Uo1)
    prob.set_step(5e-12, 4e-12)
    st = (U, Uo, Uo1, 5e-12, 4e-12)
    _check_assembly(prob, om, st, one_pass=False)
    its, _ = prob.newton_solve_species(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    R = U.copy()
    its_ref = sr.species_stage(om, R, Uo, Uo1, 5e-12, 4e-12, rtol=1e-8, max_it=20)
    G = prob.get_state().reshape(U.shape)
    d = sr.relative_difference(G, R)
    print(f"[segregated] four species: its {its} / {its_ref}, state {d}", flush=True)
    assert np.array_equal(G[:, 4], U[:, 4])
    assert its == its_ref and d.max() <= STATE_BOUND


# ---- the residual-only twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("state,mesh", [("init", "48"), ("head", "48"), ("init", "cells384")])
def test_species_residual_twin(state, mesh):
    """F_u by the residual-only kernel at ANOTHER state than the matrix's: F_u against the oracle, F_phi exactly 0, the
    matrix bit for bit what it was."""
    prob, om, st = _context(state, mesh=mesh, multigrid=False, weights=0, perturb=True)
    U, Uo, Uo1, dt, dto = st
    iu, ip = sr.block_indices(U.size, 3)
    prob.jacobian()
    J_before = prob.jacobian_csr()
    U2 = U.copy()
    U2[:, :2] += 0.02 * np.cos(np.arange(prob.nv))[:, None]
    prob.set_state(U2, Uo, Uo1)
    before = prob.segregated_stats()
    assert prob.species_assembly(jacobian=False) is True
    F = prob.residual_vector()
    Fo = om.residual_jacobian(U2, Uo, Uo1, dt, dto)[0]
    launched = prob.launched_assembly()["residual"]
    print(f"[segregated] residual twin {state} {mesh}: F_u {_rel(F[iu], Fo[iu]):.2e}, launched {launched}", flush=True)
    assert np.all(F[ip] == 0.0) and _rel(F[iu], Fo[iu]) <= 1e-11
    assert (prob.jacobian_csr() != J_before).nnz == 0
    assert launched["variant"] == "lds-patches/one-pass" and launched["launches"] == 1
    assert prob.segregated_stats()["one_pass_assemblies"] == before["one_pass_assemblies"] + 1


def test_species_newton_final_check_is_residual_only():
    """The second solve of a kind expects to converge where the first did and checks there with the twin."""
    prob, om, st = _context("init")
    U = prob.get_state()
    its, _ = prob.newton_solve_species(rtol=1e-8, ksp_rtol=1e-10)
    first = prob.get_state()
    prob.set_state(U, U, U)
    its2, _ = prob.newton_solve_species(rtol=1e-8, ksp_rtol=1e-10)
    res = prob.launched_assembly()["residual"]
    assert its2 == its and res["variant"] == "lds-patches/one-pass" and res["launches"] == 1
    assert np.abs(prob.get_state() - first).max() <= 1e-12 * np.abs(first).max()
    # a wrong guess (a loose solve converged after one update) assembles the Jacobian after all and goes on
    prob.set_state(U, U, U)
    assert prob.newton_solve_species(atol=0.0, rtol=0.5)[0] == 1
    prob.set_state(U, U, U)
    before = prob.segregated_stats()["one_pass_assemblies"]
    its3, _ = prob.newton_solve_species(rtol=1e-8, ksp_rtol=1e-10)
    assert its3 == its and prob.segregated_stats()["one_pass_assemblies"] == before + its + 2
    assert np.abs(prob.get_state() - first).max() <= 1e-12 * np.abs(first).max()


# ---- the block products --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["init", "head", "recombination", "four-species"])
def test_block_products_against_the_matrix(case):
    """y = J_uu x_u and y = J_phiphi x_phi against the host product with the blocks of ``jacobian_csr()`` <= 1e-11
    (DESIGN section 5), exact zeros on the other block's entries.  The streamer model has a structurally zero species
    plane (the product skips it), the recombining one has none, the four-species model five equations."""
    if case == "recombination":
        from fedm_amd.cases import streamer
        from lfa_models import recombining_streamer_problem
        msh = streamer.mesh(48, 4.0)
        prob = recombining_streamer_problem(msh.coords, msh.cells)
        st = _head_arrays(prob.coords, prob.nv)
        prob.set_state(st[0], st[1], st[2])
        prob.set_step(st[3], st[4])
    elif case == "four-species":
        import test_gpu_preconditioner as tp
        prob = tp.build("four-species")[0]
    else:
        prob, _, _ = _context(case, multigrid=False, weights=0, perturb=True)
    n_eq = prob.n_eq
    kept, zero = prob.plane_masks()
    assert (zero != 0) == (case in ("init", "head"))
    prob.jacobian()
    J = prob.jacobian_csr()
    iu, ip = sr.block_indices(prob.n, n_eq)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(prob.n)
    for which, rows, other, block in (("species", iu, ip, sr.species_block(J, n_eq)),
                                      ("potential", ip, iu, sr.potential_block(J, n_eq))):
        y = prob.block_product(which, x).reshape(-1)
        ref = block @ x[rows]
        e = np.abs(y[rows] - ref).max() / np.abs(ref).max()
        print(f"[segregated] product {case} {which}: {e:.2e} (zero planes {zero:#x})", flush=True)
        assert np.all(y[other] == 0.0)
        assert e <= 1e-11
    # the species product does not see the potential entries of x, nor the potential product the species entries
    x2 = x.copy()
    x2[ip] = rng.standard_normal(ip.size)
    assert np.array_equal(prob.block_product("species", x2), prob.block_product("species", x))


def test_time_kernel_kinds_6_and_7():
    prob, om, st = _context("init", multigrid=False, weights=0)
    t = {k: prob.time_kernel(k, 5) for k in (0, 2)}
    prob.jacobian()
    J = prob.jacobian_csr()
    t.update({k: prob.time_kernel(k, 5) for k in (6, 7)})
    print(f"[segregated] time_kernel on the 48 mesh: {t}", flush=True)
    assert all(np.isfinite(v) and v > 0.0 for v in t.values())
    assert prob.launched_assembly()["residual"]["launches"] == 1           # kind 7 is the residual-only assembly
    iu, ip = sr.block_indices(prob.n, 3)
    J6 = prob.jacobian_csr().tocsr()
    assert (J6[ip] != J.tocsr()[ip]).nnz == 0                                # kind 6 leaves the potential row alone
    # the fallback's volume kernel (four species) is timed as well
    import test_gpu_preconditioner as tp
    four = tp.build("four-species")[0]
    assert four.time_kernel(6, 3) > 0.0
    assert four.launched_assembly()["jacobian"]["variant"] == "lds-patches"


# ---- the linear solve ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state,weights,ksp_rtol", [("init", 6, 1e-5), ("init", 6, 1e-10), ("head", 6, 1e-5),
                                                    ("head", 6, 1e-10), ("head", 0, 1e-5), ("head", 0, 1e-10)])
def test_species_linear_solve_true_residual(state, weights, ksp_rtol):
    """J_uu x = -F_u through the call the species Newton makes (``species_linear_solve``).  Degree-6 polynomial: a few
    steps (below the 8-step boundary of the coupled loop's fused update); point-block Jacobi: beyond it.  (x is read
    from the device: the difference of two states would carry the rounding of u + x, 7e-15 / |x| -- more than 1e-10
    in the initial state, which hardly moves in 5 ps.)"""
    prob, om, st = _context(state, multigrid=False, weights=weights)
    n_eq = 3
    iu, ip = sr.block_indices(st[0].size, n_eq)
    F, J = _species_assembly(prob)
    Juu, b = sr.species_block(J, n_eq), -F[iu]
    u0 = prob.get_state()
    x, steps, reported, code = prob.species_linear_solve(-F, ksp_rtol=ksp_rtol)
    tol = ksp_rtol * np.linalg.norm(b)
    true = np.linalg.norm(Juu @ x[iu] - b)
    print(f"[segregated] linear {state} weights {weights} ksp_rtol {ksp_rtol:.0e}: code {code}, {steps} steps, "
          f"true / tol {true / tol:.4f}, reported / tol {reported / tol:.4f}", flush=True)
    assert code == 0 and np.all(x[ip] == 0.0)
    assert np.array_equal(prob.get_state(), u0)                      # the hook does not touch the state
    if weights == 6:
        assert 1 <= steps <= 8               # this side of the 8-step boundary of the coupled loop's fused update
    elif ksp_rtol == 1e-10:
        assert steps > 8                     # ... and beyond it
    assert true <= FIXED[ksp_rtol] * tol
    # the Newton loop makes the same solve: one update from here is u0 + x
    with pytest.raises(RuntimeError, match="maximum"):
        prob.newton_solve_species(rtol=1e-300, atol=0.0, max_it=1, ksp_rtol=ksp_rtol)
    assert prob.last_report.linear_iterations == steps
    moved = prob.get_state().reshape(-1) - u0.reshape(-1)
    assert np.all(moved[ip] == 0.0)
    assert np.abs(moved - x).max() <= 4.0 * np.finfo(float).eps * np.abs(u0).max()


# ---- the species Newton --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["init", "head"])
def test_species_newton_against_the_restatement(state):
    prob, om, st = _context(state)
    U, Uo, Uo1, dt, dto = st
    U = prob.get_state().reshape(U.shape)     # (setting up the multigrid has put the boundary values into the state)
    its, _ = prob.newton_solve_species(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    G = prob.get_state().reshape(U.shape)
    R = U.copy()
    rep = {}
    its_ref = sr.species_stage(om, R, Uo, Uo1, dt, dto, rtol=1e-8, max_it=20, report=rep)
    d = sr.relative_difference(G, R)
    r = prob.last_report
    print(f"[segregated] newton {state}: its {its} / {its_ref}, state {d}, |F_u| {r.fnorm0:.6e} -> {r.fnorm:.3e} "
          f"(restatement {rep['residual_history'][0]:.6e} -> {rep['residual_history'][-1]:.3e})", flush=True)
    assert np.array_equal(G[:, 2], U[:, 2])                  # bit-identical potential
    assert its == its_ref and d.max() <= STATE_BOUND
    assert r.fnorm0 == pytest.approx(rep["residual_history"][0], rel=1e-9)     # the species norm, not the full one
    s = prob.segregated_stats()
    assert s["species_solves"] == 1 and s["newton_iterations"] == its and s["krylov_steps"] == r.linear_iterations
    assert s["one_pass_assemblies"] == its + 1 and s["fallback_assemblies"] == 0


def test_species_newton_branches():
    prob, om, st = _context("init")
    U = st[0]
    # atol: converged at iteration 0
    its, _ = prob.newton_solve_species(atol=1e300, rtol=1e-8)
    assert its == 0 and prob.last_report.converged
    # rtol: a loose one ends after the first update
    its, _ = prob.newton_solve_species(atol=0.0, rtol=0.5, max_it=20)
    assert its == 1
    # max_it
    prob.set_state(U, U, U)
    with pytest.raises(RuntimeError, match="maximum"):
        prob.newton_solve_species(atol=0.0, rtol=1e-300, stol=0.0, max_it=2)
    assert prob.last_report.iterations == 2 and not prob.last_report.converged
    # NaN in a species entry
    V = U.copy()
    V[prob.nv // 2, 1] = np.nan
    prob.set_state(V, U, U)
    with pytest.raises(RuntimeError, match="(?i)nan"):
        prob.newton_solve_species()


# ---- the potential -------------------------------------------------------------------------------------------------
def test_poisson_update_against_the_direct_solve():
    prob, om, st = _context("head")
    U, Uo, Uo1, dt, dto = st
    prob.profile(True)                                        # counts the assemblies by kind
    its = prob.poisson_update(rtol=1e-13)
    first = prob.profile_read()
    G = prob.get_state().reshape(U.shape)
    R = U.copy()
    sr.potential_stage(om, R, Uo, Uo1, dt, dto)
    e = _rel(G[:, 2], R[:, 2])
    print(f"[segregated] poisson_update: {its} CG steps, potential {e:.2e}, assemblies {first}", flush=True)
    assert its > 0 and prob.last_poisson_iterations == its
    assert np.array_equal(G[:, :2], U[:, :2])                 # bit-identical species
    assert e < 1e-9
    # from another state: no Jacobian assembly after the first
    U2 = U.copy()
    U2[:, 1] += 0.3
    U2[:, 2] *= 0.9
    prob.set_state(U2, Uo, Uo1)
    prob.poisson_update(rtol=1e-13)
    second = prob.profile_read()
    R2 = U2.copy()
    sr.potential_stage(om, R2, Uo, Uo1, dt, dto)
    assert _rel(prob.get_state().reshape(U.shape)[:, 2], R2[:, 2]) < 1e-9
    assert second["assembly_FJ"][1] == first["assembly_FJ"][1]            # no Jacobian assembly
    assert second["assembly_F"][1] == first["assembly_F"][1] + 1          # one residual-only assembly
    s = prob.segregated_stats()
    assert s["poisson_updates"] == 2 and s["cg_iterations"] >= its


def test_poisson_update_without_a_hierarchy():
    prob, om, st = _context("init", multigrid=False, weights=0)
    U, Uo, Uo1, dt, dto = st
    V = U.copy()
    V[:, 2] = 0.0
    prob.set_state(V, Uo, Uo1)
    its = prob.poisson_update(rtol=1e-13)
    e = _rel(prob.get_state().reshape(U.shape)[:, 2], U[:, 2])
    print(f"[segregated] poisson_update, Jacobi: {its} CG steps, potential {e:.2e}", flush=True)
    assert e < 1e-9


# ---- whole steps ---------------------------------------------------------------------------------------------------
def test_five_steps_against_five_restated_steps():
    prob, om, st = _context("init")
    U = st[0].copy()
    Uo, Uo1 = U.copy(), U.copy()
    dt, dto = 5e-12, 1e30
    for _ in range(5):
        prob.shift_state()
        prob.set_step(dt, dto)
        prob.segregated_solve(poisson_rtol=1e-12, rtol=1e-10, max_it=20, ksp_rtol=1e-12)
        Uo1[:] = Uo
        Uo[:] = U
        sr.segregated_step(om, U, Uo, Uo1, dt, dto, rtol=1e-10, max_it=20)
        dto = dt
    d = sr.relative_difference(prob.get_state().reshape(U.shape), U)
    print(f"[segregated] five steps: difference to the restatement {d} (bound {FIVE_STEP_BOUND['init']:.1e})", flush=True)
    assert d.max() <= FIVE_STEP_BOUND["init"]


def test_through_the_solver_and_the_stepper():
    from fedm_amd.cases import streamer
    msh = streamer.mesh(48, 4.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    stp = streamer.Stepper(prob, coupling="uncoupled")
    stp.initialise()
    for _ in range(10):
        stp.step()
    rows = np.array(stp.log_rows())
    s = prob.segregated_stats()
    print(f"[segregated] stepper: t {stp.t:.3e}, {len(rows)} log rows, {s}", flush=True)
    assert stp.steps == 10 and len(rows) >= 10 and np.all(np.isfinite(rows))
    assert s["poisson_updates"] >= 10 and s["species_solves"] >= 10 and s["fallback_assemblies"] == 0
    assert prob.solver_path_stats()["solves"] == 0                  # the coupled GMRES never ran
    # a forced failure is retried with a halved step
    stp.solver.parameters["maximum_iterations"] = 1
    stp.solver.parameters["relative_tolerance"] = 1e-14
    stp.dt_min = stp.dt.time_step / 3.0
    dt_before = stp.dt.time_step
    with pytest.raises(SystemExit):
        stp.step()
    assert stp.dt.time_step == pytest.approx(0.25 * dt_before)      # halved twice, then below dt_min


def test_coexistence_with_the_coupled_solve():
    prob, om, st = _context("init")
    U = st[0]
    for _ in range(2):
        prob.shift_state()
        prob.segregated_solve(rtol=1e-8, ksp_rtol=1e-10)
    start = prob.get_state().reshape(U.shape)
    prob.set_state(start, start, start)
    prob.set_step(5e-12, 1e30)
    prob.solver_path_stats(reset=True)
    prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    paths_after_segregated = prob.solver_path_stats()
    mixed = prob.get_state().reshape(U.shape)
    prob.jacobian()
    Jo = om.residual_jacobian(mixed, start, start, 5e-12, 1e30)[1]
    eJ = abs(prob.jacobian_csr() - Jo).max() / abs(Jo).max()
    fresh, _, _ = _context("init")
    assert all(v == 0 for v in fresh.segregated_stats().values())
    fresh.set_state(start, start, start)
    fresh.solver_path_stats(reset=True)
    fresh.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    d = sr.relative_difference(mixed, fresh.get_state().reshape(U.shape))
    print(f"[segregated] coexistence: J {eJ:.2e}, state {d}", flush=True)
    assert eJ <= 1e-10 and d.max() <= STATE_BOUND
    assert all(v == 0 for v in fresh.segregated_stats().values())     # a coupled-only context counts nothing here
    # ... and the coupled driver ends the same way whether segregated steps ran on the context before or not.  Its
    # step and cycle counts are not compared: at ksp_rtol 1e-10 these solves end within a step of the restart length
    # (measured: 30 steps a solve in one context, 32 with a second cycle in the other), where the summation order of the
    # assembly's atomics decides.
    paths = fresh.solver_path_stats()
    print(f"[segregated] coexistence: paths {({k: v for k, v in paths.items() if v})} against "
          f"{({k: v for k, v in paths_after_segregated.items() if v})}", flush=True)
    assert paths["solves"] > 0
    for key in ("solves", "newton_max_it", "exhausted", "breakdowns"):
        assert paths[key] == paths_after_segregated[key], key


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    prob, om, st = _context("init")
    before = (prob.launched_assembly(), prob.segregated_stats())
    prob.set_krylov_scaling("rows")
    with pytest.raises(RuntimeError, match="rows"):
        prob.newton_solve_species()
    prob.set_krylov_scaling("none")
    prob.set_preconditioner_side("left")
    with pytest.raises(RuntimeError, match="left"):
        prob.newton_solve_species()
    prob.set_preconditioner_side("right")
    assert (prob.launched_assembly(), prob.segregated_stats()) == before
    assert np.array_equal(prob.get_state().reshape(st[0].shape), st[0])


def test_model_without_a_poisson_row_is_refused():
    from fedm_amd.cases import time_of_flight as tof
    prob, _ = tof.device_problem(16, 16, 1.0e-3, 1.0e-3)
    for call in (prob.poisson_update, prob.newton_solve_species, lambda: prob.time_kernel(6, 1)):
        with pytest.raises(RuntimeError, match="Poisson"):
            call()
    assert all(v == 0 for v in prob.segregated_stats().values())


def test_lmea_context_is_refused():
    import contextlib
    import io
    from fedm_amd.cases import glow_discharge as gdc
    with contextlib.redirect_stdout(io.StringIO()):
        gd = gdc.Case(nx=40, ny=40, T_final=1.0)
    for call in (gd.prob.poisson_update, gd.prob.newton_solve_species, lambda: gd.prob.time_kernel(6, 1)):
        with pytest.raises(RuntimeError, match="LMEA"):
            call()
    assert all(v == 0 for v in gd.prob.segregated_stats().values())
