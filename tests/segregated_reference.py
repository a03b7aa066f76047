"""Float64 restatement of the segregated (uncoupled) time step -- test infrastructure.

The reference solves the potential on its own with the densities frozen (``Poisson_solver``,
fedm/functions.py:1154-1161) and the species among themselves with the field frozen (``Source_term`` /
``Energy_Source_term`` with ``coupling='uncoupled'``, :777-843, :845-912).  Restated here by block extraction
from the oracle's ``residual_jacobian`` -- no new physics:

* potential stage: one assembly at the state as it stands, ``J[ip][:, ip] dphi = -F[ip]`` solved directly (the
  Poisson rows are linear in the potential; the Dirichlet rows are identity rows with ``F = phi - g``);
* species stage: Newton with the rules of ``oracle.newton.newton_solve`` on ``J[iu][:, iu]``, ``F[iu]``, norms over
  the species entries, the potential entries never written.

``solver(...)`` returns a callable for ``oracle.streamer.run(solver=...)``.  The block helpers take any scipy
matrix in the interleaved dof order (dof = vertex * n_eq + component, potential last), so they work on the
device's ``jacobian_csr()`` as well.  ``fault=`` plants the three mistakes the tests must be able to see.
"""
import numpy as np

from oracle.newton import NewtonDiverged, direct_solve


def block_indices(n, n_eq):
    """(species dofs, potential dofs) of a vector of n interleaved dofs."""
    dofs = np.arange(n)
    pot = dofs % n_eq == n_eq - 1
    return dofs[~pot], dofs[pot]


def species_block(J, n_eq):
    iu, _ = block_indices(J.shape[0], n_eq)
    return J.tocsr()[iu][:, iu]


def potential_block(J, n_eq):
    _, ip = block_indices(J.shape[0], n_eq)
    return J.tocsr()[ip][:, ip]


def potential_stage(model, U, Uold, Uold1, dt, dt_old):
    """The potential entries of U from the Poisson rows, the species entries of U frozen.  In place."""
    n_eq = U.shape[1]
    F, J = model.residual_jacobian(U, Uold, Uold1, dt, dt_old)
    _, ip = block_indices(F.size, n_eq)
    U[:, n_eq - 1] += direct_solve(potential_block(J, n_eq), -F[ip])


def species_stage(model, U, Uold, Uold1, dt, dt_old, rtol=1e-8, max_it=20, atol=1e-10, stol=1e-16,
                  linear_solve=None, report=None, frozen=True):
    """Newton on the species rows, the potential entries of U frozen.  In place; returns the iteration count.
    ``frozen=False`` is a planted fault: the full coupled system is solved and the potential moves."""
    n_eq = U.shape[1]
    iu, _ = block_indices(U.size, n_eq)
    rows = iu if frozen else np.arange(U.size)
    flat = U.reshape(-1)
    its, fnorm0, snorm, history = 0, None, 0.0, []
    while True:
        F, J = model.residual_jacobian(U, Uold, Uold1, dt, dt_old)
        Fu = F[rows]
        fnorm = float(np.linalg.norm(Fu))
        history.append(fnorm)
        if not np.isfinite(fnorm):
            raise NewtonDiverged("species residual norm is not finite")
        if its == 0:
            fnorm0 = fnorm
            if fnorm < atol:
                break
        elif fnorm < atol or fnorm <= rtol * fnorm0 or snorm < stol * float(np.linalg.norm(flat[rows])):
            break
        if its >= max_it:
            raise NewtonDiverged(f"no convergence in {max_it} species Newton iterations")
        Juu = J.tocsr()[rows][:, rows]
        delta = direct_solve(Juu, -Fu) if linear_solve is None else linear_solve(Juu, -Fu)
        snorm = float(np.linalg.norm(delta))
        flat[rows] += delta
        its += 1
    if report is not None:
        report["residual_history"] = history
        report["iterations"] = its
    return its


def segregated_step(model, U, Uold, Uold1, dt, dt_old, fault=None, report=None, **newton):
    """One segregated step in place from U (= Uold at the start of a step).
    fault: None | "swapped" (species first, then the potential with the NEW densities) | "unfrozen" (the potential
    moves in the species Newton) | "stale" (the species are solved with the field of the previous step; the
    potential of the old densities is stored afterwards)."""
    n_eq = U.shape[1]
    if fault is None:
        potential_stage(model, U, Uold, Uold1, dt, dt_old)
        return species_stage(model, U, Uold, Uold1, dt, dt_old, report=report, **newton)
    if fault == "swapped":
        its = species_stage(model, U, Uold, Uold1, dt, dt_old, report=report, **newton)
        potential_stage(model, U, Uold, Uold1, dt, dt_old)
        return its
    if fault == "unfrozen":
        potential_stage(model, U, Uold, Uold1, dt, dt_old)
        return species_stage(model, U, Uold, Uold1, dt, dt_old, report=report, frozen=False, **newton)
    if fault == "stale":
        W = U.copy()
        potential_stage(model, W, Uold, Uold1, dt, dt_old)
        its = species_stage(model, U, Uold, Uold1, dt, dt_old, report=report, **newton)
        U[:, n_eq - 1] = W[:, n_eq - 1]
        return its
    raise ValueError(f"unknown fault {fault!r}")


def solver(fault=None, counts=None, **newton):
    """A ``solver`` for ``oracle.streamer.run``; ``counts`` (a list) collects the species Newton iterations."""
    def solve(model, Uw, U_old, U_old1, dt, dt_old):
        its = segregated_step(model, Uw, U_old, U_old1, dt, dt_old, fault=fault, **newton)
        if counts is not None:
            counts.append(its)
    return solve


def relative_difference(A, B):
    """Per component: max |A - B| over the component's largest |B|."""
    return np.abs(A - B).max(axis=0) / np.abs(B).max(axis=0)
