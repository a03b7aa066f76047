"""The float64 restatement of the field-split preconditioner (tests/fieldsplit_reference.py) against dense linear
algebra, on the oracle's Jacobian of the streamer model on a 10 x 10 mesh (no GPU): the sweeps are the closed-form
polynomial in S = Duu^-1 J_uu, the cycles are their dense error-propagation formulas, V(nu, nu) is symmetric, and the
lagged coupling differs from the plain one by exactly the cycle of the lag's product.  The GPU file
(test_gpu_preconditioner.py) then holds the device to this restatement."""
import numpy as np
import pytest
import scipy.sparse as sp

from fieldsplit_reference import PERTURBATIONS, FieldSplit, Multigrid, balanced_rhs, rel_diff, sweep_polynomial


@pytest.fixture(scope="module")
def system():
    """(J, Dirichlet mask of the vertices, potential block with its Dirichlet rows and columns made identity)."""
    from oracle import streamer as ost
    from oracle.mesh import rectangle_right
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, 10, 10)
    om = ost.build(mesh)
    U0 = ost.initial_state(om)
    rng = np.random.default_rng(2)
    U = U0 + np.c_[0.05 * rng.standard_normal(mesh.nv), 0.3 * rng.standard_normal(mesh.nv), np.zeros(mesh.nv)]
    _, J = om.residual_jacobian(U, U0, U0, 5e-12, 4e-12)
    J = sp.csr_matrix(J)
    fixed = np.zeros(mesh.nv, dtype=bool)
    fixed[np.asarray(om.dirichlet_dofs) // 3] = True
    K = J[2::3][:, 2::3].tolil()
    for i in np.nonzero(fixed)[0]:
        K[i, :] = 0.0
        K[:, i] = 0.0
        K[i, i] = 1.0
    return J, fixed, sp.csr_matrix(K)


def _two_levels(K, fixed, size=4):
    """A smoothed-aggregation pair (aggregates of `size` consecutive free vertices): [(K, P), (P^T K P, None)]."""
    free = np.nonzero(~fixed)[0]
    T = sp.csr_matrix((np.ones(free.size), (free, np.arange(free.size) // size)),
                      shape=(K.shape[0], (free.size + size - 1) // size))
    DinvK = sp.diags(1.0 / K.diagonal()) @ K
    P = sp.csr_matrix(T - (2.0 / 3.0) * (DinvK @ T) / np.abs(DinvK).sum(axis=1).max())
    P = sp.diags((~fixed).astype(float)) @ P
    return [(K, P), (sp.csr_matrix(P.T @ K @ P), None)]


def _dense(op, n):
    return np.column_stack([op(e) for e in np.eye(n)])


@pytest.mark.parametrize("weights", [np.array([0.9, 1.1]), "cheb6", "cheb8", np.array([0.7, 1.3, 0.8, 1.6, 0.5])])
def test_species_sweeps_are_the_closed_form_polynomial_in_S(system, weights):
    from fedm_amd.device import chebyshev_weights
    J, fixed, K = system
    if isinstance(weights, str):
        weights = chebyshev_weights(int(weights[4:]))
    fs = FieldSplit(J, 2, Multigrid([(K, None)]), weights)
    g = np.random.default_rng(0).standard_normal(fs.su.size)
    z, prev = fs.sweeps(g, fs.S)
    S = fs.S.toarray()
    q = sweep_polynomial(weights)
    zq = np.zeros_like(g)
    for c in q[::-1]:                                  # Horner
        zq = S @ zq + c * g
    assert np.abs(z - zq).max() <= 1e-12 * np.abs(zq).max()
    # the lagged coupling's operand is the iterate before the last sweep: the polynomial of one degree less
    zp = np.zeros_like(g)
    for c in sweep_polynomial(weights[:-1])[::-1]:
        zp = S @ zp + c * g
    assert np.abs(prev - zp).max() <= 1e-12 * np.abs(zp).max()


def test_species_block_jacobi_is_the_inverse_of_the_diagonal_blocks(system):
    J, fixed, K = system
    fs = FieldSplit(J, 2, Multigrid([(K, None)]), [0.8])
    t = balanced_rhs(J, 2, np.random.default_rng(1))
    z = fs.apply(t)
    Juu = J[fs.su][:, fs.su].toarray()
    D = np.zeros_like(Juu)
    for v in range(fs.nv):
        D[2 * v:2 * v + 2, 2 * v:2 * v + 2] = Juu[2 * v:2 * v + 2, 2 * v:2 * v + 2]
    zu = np.linalg.solve(D, t[fs.su])
    assert np.abs(z[fs.su] - zu).max() <= 1e-12 * np.abs(zu).max()
    b = t[fs.ph] - J[fs.ph][:, fs.su] @ zu
    assert np.abs(z[fs.ph] - np.linalg.solve(K.toarray(), b)).max() <= 1e-9 * np.abs(z[fs.ph]).max()


@pytest.mark.parametrize("cycle", ["V(1,1)", "V(2,2)", "V(0,2)", "polynomial"])
def test_two_level_cycle_is_its_dense_formula(system, cycle):
    """I - M A = post (I - P Ac^-1 P^T A) pre with the exact coarse inverse; pre / post the smoothers' error
    propagators: (I - omega Dinv A)^nu, none for V(0, nu), prod (I - w_i Dinv A) in order / backwards."""
    J, fixed, K = system
    levels = _two_levels(K, fixed)
    n = K.shape[0]
    A = K.toarray()
    Dinv = np.diag(1.0 / np.diag(A))
    I = np.eye(n)
    if cycle == "polynomial":
        w = np.array([[0.6, 1.4]])
        mg = Multigrid(levels, nu=2, poly_weights=w)
        pre = (I - w[0, 1] * Dinv @ A) @ (I - w[0, 0] * Dinv @ A)
        post = (I - w[0, 0] * Dinv @ A) @ (I - w[0, 1] * Dinv @ A)
    else:
        nu = int(cycle[4])
        mg = Multigrid(levels, nu=nu if cycle != "V(0,2)" else -nu, omega=0.8)
        post = np.linalg.matrix_power(I - 0.8 * Dinv @ A, nu)
        pre = I if cycle == "V(0,2)" else post
    P = levels[0][1].toarray()
    Ac = P.T @ A @ P
    E = post @ (I - P @ np.linalg.solve(Ac, P.T @ A)) @ pre
    M = (I - E) @ np.linalg.inv(A)
    Md = _dense(mg.apply, n)
    assert np.abs(Md - M).max() <= 1e-10 * np.abs(M).max()


@pytest.mark.parametrize("cycle", ["V(1,1)", "V(2,2)", "polynomial"])
def test_symmetric_cycles_are_symmetric(system, cycle):
    J, fixed, K = system
    levels = _two_levels(K, fixed)
    if cycle == "polynomial":
        mg = Multigrid(levels, nu=2, poly_weights=np.array([[0.6, 1.4]]))
    else:
        mg = Multigrid(levels, nu=int(cycle[2]), omega=0.85)
    M = _dense(mg.apply, K.shape[0])
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    # (V(0, nu) is not: the test can tell)
    M0 = _dense(Multigrid(levels, nu=-1, omega=0.85).apply, K.shape[0])
    assert np.abs(M0 - M0.T).max() > 1e-3 * np.abs(M0).max()


def test_lagged_minus_plain_coupling_is_the_cycle_of_the_lag(system):
    """b_phi(lagged) - b_phi(plain) = J_phi,u (z_u - z_prev): the potentials differ by the cycle of that vector, the
    species not at all."""
    from fedm_amd.device import chebyshev_weights
    J, fixed, K = system
    mg = Multigrid(_two_levels(K, fixed), nu=1, omega=0.85)
    w = chebyshev_weights(6)
    lag, plain = FieldSplit(J, 2, mg, w, lagged=True), FieldSplit(J, 2, mg, w, lagged=False)
    t = balanced_rhs(J, 2, np.random.default_rng(3))
    za, zb = lag.apply(t), plain.apply(t)
    assert np.array_equal(za[lag.su], zb[lag.su])
    z_u, prev = lag.sweeps(lag.dinv_u(t[lag.su]), lag.S)
    d = mg.apply(lag.Jpu @ (z_u - prev))
    assert np.abs((za - zb)[lag.ph] - d).max() <= 1e-11 * np.abs(za[lag.ph]).max()
    assert np.abs(d).max() > 1e-6 * np.abs(za[lag.ph]).max()          # (the lag does change the preconditioner)


def test_upper_order_solves_the_upper_block_system_with_exact_blocks(system):
    """With one weight (block Jacobi on species) and a one-level hierarchy (the exact inverse), the upper order is the
    exact inverse of [[Duu, J_u,phi], [0, K]]."""
    J, fixed, K = system
    fs = FieldSplit(J, 2, Multigrid([(K, None)]), [1.0], order="upper")
    t = balanced_rhs(J, 2, np.random.default_rng(4))
    z = fs.apply(t)
    Juu = J[fs.su][:, fs.su].toarray()
    D = np.zeros_like(Juu)
    for v in range(fs.nv):
        D[2 * v:2 * v + 2, 2 * v:2 * v + 2] = Juu[2 * v:2 * v + 2, 2 * v:2 * v + 2]
    r = np.zeros_like(t)
    r[fs.su] = D @ z[fs.su] + fs.Jup @ z[fs.ph]
    r[fs.ph] = K @ z[fs.ph]
    scale = np.abs(fs.Jup @ z[fs.ph]).max() + np.abs(t).max()
    assert np.abs(r - t).max() <= 1e-12 * scale


def test_emulated_precision_and_every_perturbation_change_the_result(system):
    from fedm_amd.device import chebyshev_weights
    J, fixed, K = system
    fs = FieldSplit(J, 2, Multigrid(_two_levels(K, fixed), nu=1, omega=0.85), chebyshev_weights(6))
    t = balanced_rhs(J, 2, np.random.default_rng(5))
    z = fs.apply(t)
    e = rel_diff(fs.apply(t, "emulate"), z, 3)
    assert 1e-8 < e < 1e-2, e
    for p in PERTURBATIONS:
        assert rel_diff(fs.apply(t, perturb=p), z, 3) > 1e-4, p
