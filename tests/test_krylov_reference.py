"""The float64 restatement of the solvers (tests/krylov_reference.py) against ``scipy.sparse.linalg.spsolve`` on
Jacobians the oracle assembles (no GPU), and the negative controls of tests/test_gpu_krylov.py: four deliberate faults of
the restatement must each miss that file's assertion 1 (true residual against the tolerance) or 2 (drift of the
recurrence) by more than 100x its bound -- proof that the bounds would catch such a fault in the device's driver."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import krylov_reference as kr
from fieldsplit_reference import FieldSplit, Multigrid


@pytest.fixture(scope="module")
def system():
    """The oracle's streamer model on a 12 x 12 mesh, a perturbed early state: (model, states, J, F, field split)."""
    from fedm_amd import amg
    from fedm_amd.device import chebyshev_weights
    from oracle import streamer as ost
    from oracle.mesh import rectangle_right
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, 12, 12)
    om = ost.build(mesh)
    U0 = ost.initial_state(om)
    rng = np.random.default_rng(2)
    U = U0 + np.c_[0.05 * rng.standard_normal(mesh.nv), 0.3 * rng.standard_normal(mesh.nv), np.zeros(mesh.nv)]
    F, J = om.residual_jacobian(U, U0, U0, 5e-12, 4e-12)
    J = sp.csr_matrix(J)
    fixed = np.zeros(mesh.nv, dtype=bool)
    fixed[np.asarray(om.dirichlet_dofs) // 3] = True
    K = J[2::3][:, 2::3].tolil()
    for i in np.nonzero(fixed)[0]:
        K[i, :] = 0.0
        K[:, i] = 0.0
        K[i, i] = 1.0
    levels = amg.build_hierarchy(sp.csr_matrix(K), theta=0.08, max_coarse=40, fixed=fixed, coords=mesh.coords)
    fs = FieldSplit(J, 2, Multigrid(levels, nu=1, omega=0.85), chebyshev_weights(6))
    return om, (U, U0), J, np.asarray(F).ravel(), fs


def _true(J, x, b):
    return float(np.linalg.norm(J @ x - b))


# (a preconditioner rounded to single precision defines no left-preconditioned system below 1e-7: the emulation is on
# the right only, like the device's default)
@pytest.mark.parametrize("side,precision", [("right", "float64"), ("left", "float64"), ("right", "emulate")])
@pytest.mark.parametrize("restart", [30, 4, 1])
def test_gmres_against_spsolve(system, side, restart, precision):
    om, _, J, F, fs = system
    b = -F
    M = lambda t: fs.apply(t, precision)
    rtol = 1e-10 if precision == "float64" else 1e-8
    res = kr.gmres(J, b, M, side=side, restart=restart, rtol=rtol, max_it=3000)
    assert res.code == kr.CONVERGED and res.its == len(res.history)
    r, bb = J @ res.x - b, b
    if side == "left":
        r, bb = M(r), M(b)
    tol = rtol * np.linalg.norm(bb)
    true = np.linalg.norm(r)
    assert true <= tol * (1 + 1e-6)
    assert abs(true - res.rnorm) <= 1e-12 * np.linalg.norm(bb)       # full re-orthogonalisation: no drift
    if restart < res.its:
        assert res.cycles >= 2
    if precision == "float64" and side == "right":
        exact = spla.spsolve(sp.csc_matrix(J), b)
        # |J (x - exact)| <= tol: the solution of the same system
        assert np.linalg.norm(J @ (res.x - exact)) <= tol * (1 + 1e-6) + 1e-12 * np.linalg.norm(b)


def test_gmres_with_block_jacobi_needs_many_cycles(system):
    om, _, J, F, fs = system
    M = kr.block_jacobi(J, 3)
    res = kr.gmres(J, -F, M, side="left", restart=30, rtol=1e-8, max_it=5000)
    assert res.code == kr.CONVERGED and res.cycles >= 2 and res.its > 30
    assert np.linalg.norm(M(J @ res.x + F)) <= 1e-8 * np.linalg.norm(M(-F)) * (1 + 1e-6)


def test_gmres_endings(system):
    om, _, J, F, fs = system
    M = fs.apply
    res = kr.gmres(J, np.zeros(J.shape[0]), M)
    assert res.code == kr.CONVERGED and res.its == 0 and res.cycles == 0 and not res.x.any()
    res = kr.gmres(J, -F, M, rtol=1e-5, atol=2.0 * np.linalg.norm(F))
    assert res.code == kr.CONVERGED and res.its == 0 and not res.x.any()
    full = kr.gmres(J, -F, M, rtol=1e-10)
    assert full.its >= 4
    res = kr.gmres(J, -F, M, rtol=1e-10, max_it=2)
    assert res.code == kr.DIVERGED_LINEAR and res.its == 2
    assert abs(res.rnorm - _true(J, res.x, -F)) <= 1e-12 * np.linalg.norm(F)     # the true norm is reported
    res = kr.gmres(J, -F, M, rtol=1e-10, restart=3, max_it=4)                      # inside the second cycle
    assert res.code == kr.DIVERGED_LINEAR and res.its == 4 and res.cycles == 2
    assert abs(res.rnorm - _true(J, res.x, -F)) <= 1e-12 * np.linalg.norm(F)
    b = -F.copy()
    b[5] = np.nan
    assert kr.gmres(J, b, M).code == kr.DIVERGED_NAN
    # a right-hand side in an invariant subspace: happy breakdown, the exact solution of the small system
    Jd = sp.diags(np.arange(1.0, 9.0)).tocsr()
    e = np.zeros(8)
    e[[1, 4]] = 1.0
    res = kr.gmres(Jd, e, rtol=1e-14)
    assert res.its == 2 and np.allclose(res.x, e / np.arange(1.0, 9.0), rtol=1e-13, atol=0)


def test_newton_loop_against_the_oracle(system):
    """The restated Newton loop with a direct solve walks the oracle's own Newton iteration; with restated GMRES at
    1e-10 it reaches the same state; its endings are PETSc's."""
    from oracle.newton import newton_solve
    om, (U, U0), J, F, fs = system

    def rj(u):
        Fu, Ju = om.residual_jacobian(u.reshape(U.shape), U0, U0, 5e-12, 4e-12)
        return np.asarray(Fu).ravel(), sp.csr_matrix(Ju)
    ref = kr.newton(rj, U.ravel(), rtol=1e-9)
    Uo = U.copy()
    its, ok = newton_solve(om, Uo, U0, U0, 5e-12, 4e-12, 1e-9, 50)
    assert ok and ref.code == kr.CONVERGED and ref.its == its
    assert np.abs(ref.u - Uo.ravel()).max() <= 1e-9 * np.abs(Uo).max()

    def krylov(Jk, b):
        return kr.gmres(Jk, b, FieldSplit(Jk, 2, fs.mg, fs.weights).apply, rtol=1e-10)
    it = kr.newton(rj, U.ravel(), rtol=1e-9, linear_solve=krylov)
    assert it.code == kr.CONVERGED and it.linear_its >= it.its >= 1
    assert np.abs(it.u - ref.u).max() <= 1e-8 * np.abs(ref.u).max()
    # endings: max_it; atol at iteration 0 leaves the state alone; stol stops at the iteration whose update is small
    assert kr.newton(rj, U.ravel(), rtol=1e-9, max_it=1).code == kr.DIVERGED_MAX_IT
    done = kr.newton(rj, ref.u, atol=10.0 * ref.fnorms[-1] + 1e-300)
    assert done.code == kr.CONVERGED and done.its == 0 and np.array_equal(done.u, ref.u)
    assert len(ref.snorms) >= 2
    s2 = ref.snorms[1]
    assert kr.newton(rj, U.ravel(), rtol=1e-30, atol=0.0, stol=s2 * 1.01, max_it=6).its == 2
    assert kr.newton(rj, U.ravel(), rtol=1e-30, atol=0.0, stol=s2 * 0.99, max_it=6).its >= 3


# ---- negative controls ---------------------------------------------------------------------------------------------
# fault: what makes it show (restarts for the faults of the cycle bookkeeping)
CONTROLS = {"drop_last_column": dict(restart=30), "skip_rotation": dict(restart=30),
            "no_accumulate": dict(restart=3), "stale_y": dict(restart=3)}


@pytest.mark.parametrize("fault", kr.FAULTS)
def test_faults_miss_the_bounds_of_the_gpu_file_by_100x(system, fault):
    """The faulty restatement still 'converges' by its own recurrence; the float64 residual must give it away against
    the bounds the device is held to (test_gpu_krylov.G_BOUND / DRIFT_BOUND / FIXED) at one of the two tolerances."""
    import test_gpu_krylov as tg
    om, _, J, F, fs = system
    b = -F
    bnorm = np.linalg.norm(b)
    worst = 0.0
    for rtol in (1e-5, 1e-10):
        good = kr.gmres(J, b, fs.apply, rtol=rtol, **CONTROLS[fault])
        assert good.code == kr.CONVERGED
        assert _true(J, good.x, b) <= rtol * bnorm * (1 + tg.G_BOUND["right"]) + tg.DRIFT_BOUND["right"] * bnorm
        bad = kr.gmres(J, b, fs.apply, rtol=rtol, fault=fault, **CONTROLS[fault])
        true, tol = _true(J, bad.x, b), rtol * bnorm
        miss1 = true / (tol * max(1.0 + tg.G_BOUND["right"], tg.FIXED[rtol]) + tg.DRIFT_BOUND["right"] * bnorm)
        miss2 = (abs(true - bad.rnorm) / bnorm) / tg.DRIFT_BOUND["right"]
        worst = max(worst, miss1, miss2)
    assert worst > 100.0, worst


# ---- the inputs of the GPU table, predicted ------------------------------------------------------------------------------
class _StateRecorder:
    """Stands in for a DeviceProblem where a helper of the GPU tests sets a state: keeps what it was given."""

    def __init__(self, nv):
        self.nv = nv

    def set_state(self, *states):
        self.states = [np.asarray(s, dtype=np.float64) for s in states]

    def set_step(self, dt, dt_old):
        self.step = (dt, dt_old)


@pytest.fixture(scope="module")
def table_systems():
    """The oracle's Jacobian, residual and field split (float64 and emulated) of the two streamer contexts of
    test_gpu_krylov on ``streamer.mesh(48, 4.0)``: the initial state ("init48") and the developed head ("head48")."""
    from fedm_amd import amg
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from test_gpu_preconditioner import _head_state
    msh = streamer.mesh(48, 4.0)
    om = ost.build(OMesh(msh.coords, msh.cells))
    nv = msh.coords.shape[0]
    out = {}
    for name in ("init48", "head48"):
        if name == "init48":
            U0 = ost.initial_state(om)
            states, step = (U0, U0, U0), (5e-12, 1e30)
        else:
            rec = _StateRecorder(nv)
            _head_state(rec, msh.coords)
            states, step = rec.states, rec.step
        F, J = om.residual_jacobian(*states, *step)
        J = sp.csr_matrix(J)
        fixed = np.zeros(nv, dtype=bool)
        fixed[np.asarray(om.dirichlet_dofs) // 3] = True
        K = J[2::3][:, 2::3].tolil()
        for i in np.nonzero(fixed)[0]:
            K[i, :] = 0.0
            K[:, i] = 0.0
            K[i, i] = 1.0
        levels = amg.build_hierarchy(sp.csr_matrix(K), theta=0.08, max_coarse=40, fixed=fixed, coords=msh.coords)
        fs = FieldSplit(J, 2, Multigrid(levels, nu=1, omega=0.85), chebyshev_weights(6))
        out[name] = (J, np.asarray(F).ravel(), fs)
    return out


def _predicted(system, rtol, precision="emulate"):
    J, F, fs = system
    res = kr.gmres(J, -F, lambda t: fs.apply(t, precision), rtol=rtol, max_it=200)
    assert res.code == kr.CONVERGED
    return res.its


def test_predicted_step_counts_sit_inside_the_bands_of_the_gpu_table(table_systems):
    """The restatement (emulated preconditioner) on the oracle's systems of the table's streamer contexts: where
    test_gpu_krylov asks for a band, the predicted count lies at least 2 steps inside it; the ksp_rtol sweep on the
    developed head crosses the 8 -> 9 boundary of the fused update, so both sides occur (the two boundary cases sit ON
    the band edges by construction).  Not predicted: the glow discharge and the four-species model (no oracle-side
    hierarchy of theirs is restated), the locally refined mesh (17 k vertices: minutes of dense Krylov vectors in
    numpy), and every case at 1e-10, where the device's own count moves by several steps from run to run."""
    import test_gpu_krylov as tg
    init, head = table_systems["init48"], table_systems["head48"]
    its = {("init48", r): _predicted(init, r) for r in (1e-5,)}
    its.update({("head48", r): _predicted(head, r) for r in (1e-3, 1e-4, 1e-5, 1e-6, 3e-7, 1e-7)})
    print(f"[krylov] predicted step counts: {its}")
    lo, hi = tg.CASES["short-init48"]["its"]
    assert lo + 0 <= its[("init48", 1e-5)] <= hi - 2
    # (measured on the device: 3, 6, 8, 9, 11 steps where 3, 6, 8, 9, 10 are predicted -- and 30 and more from 1e-7 on,
    # where 12 are predicted: the recurrence's norm lags the true residual there)
    lo, hi = tg.CASES["long-head48-3e-7"]["its"]
    assert lo + 2 <= its[("head48", 3e-7)] <= hi - 2
    assert lo + 2 <= its[("head48", 1e-7)] <= hi - 2
    assert lo < its[("head48", 1e-6)] < hi
    sweep = [its[("head48", r)] for r in (1e-3, 1e-4, 1e-5, 1e-6)]
    assert sweep == sorted(sweep) and sweep[0] <= 8 and sweep[-1] >= 9          # the sweep crosses the boundary
    assert its[("head48", 1e-4)] <= 8 < 9 <= its[("head48", 1e-5)]              # ... where the table's two cases sit
    # the hint cases: a short solve of at most 4 steps ('as the last one' needs a hint <= 4), a long one >= 2 more
    assert its[("init48", 1e-5)] <= 4
    # restarts: a solve of 10 or more steps for m = 3, 5, 8
    assert its[("head48", 1e-6)] >= 10


def test_predicted_restart_cases_without_a_hierarchy(table_systems):
    """Block Jacobi on the left without a hierarchy needs more than 30 steps on the developed head (the m = 30 restart
    case) -- and many cycles at m = 1 on the initial state."""
    J, F, fs = table_systems["head48"]
    M = kr.block_jacobi(J, 3)
    res = kr.gmres(J, -F, M, side="left", restart=30, rtol=1e-5, max_it=2000)
    assert res.code == kr.CONVERGED and res.its > 32 and res.cycles >= 2
    J, F, fs = table_systems["init48"]
    res = kr.gmres(J, -F, kr.block_jacobi(J, 3), side="left", restart=1, rtol=1e-5, max_it=2000)
    assert res.code == kr.CONVERGED and res.its > 32 and res.cycles == res.its
