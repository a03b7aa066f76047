"""Float64 restatement of the row-equilibrated GMRES of ``fedm_set_krylov_scaling``, on top of
tests/krylov_reference.py and tests/fieldsplit_reference.py.

The scaling: for the DOF i = (vertex v, component r), ``s_i = sqrt(sum_c J[(v, r), (v, c)]^2)`` over row r of the
vertex's n_eq x n_eq diagonal block, ``d_i = 1 / s_i`` and ``d_i = 1`` where s_i is zero or not finite.  A scaled solve is
right-preconditioned GMRES on ``(D J) x = D b`` with the preconditioner ``t -> M(t / d)``: the operator
``D J M^-1 D^-1``, tested on ``|D (b - J x)|``.  The device runs the same iterates in the inner product
``<x, y> = sum_i d_i^2 x_i y_i`` with its vectors unscaled.

``misformulated=True`` is the trap: the operator's rows scaled, the preconditioner's input not un-scaled
(``D J M^-1 ~ D``, a spectrum over 16 decades) -- kept as a negative control.
"""
import numpy as np
import scipy.sparse as sp

import krylov_reference as kr


def diagonal_blocks(J, n_eq):
    """[vertex][row][column] of the n_eq x n_eq diagonal blocks of J."""
    J = sp.csr_matrix(J)
    nv = J.shape[0] // n_eq
    base = np.arange(nv) * n_eq
    blocks = np.empty((nv, n_eq, n_eq))
    for r in range(n_eq):
        for c in range(n_eq):
            blocks[:, r, c] = np.asarray(J[base + r, base + c]).ravel()
    return blocks


def row_norms(J, n_eq):
    """s: the 2-norm of every row of its vertex's diagonal block."""
    return np.sqrt((diagonal_blocks(J, n_eq) ** 2).sum(axis=2)).ravel()


def row_scale(J, n_eq):
    """d = 1 / s, and 1 where s is zero or not finite."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = row_norms(J, n_eq)
    d = np.ones_like(s)
    ok = np.isfinite(s) & (s > 0.0)
    d[ok] = 1.0 / s[ok]
    return d


def scaled_residual(J, x, b, d):
    """(|D (J x - b)|, |D b|) in float64."""
    return float(np.linalg.norm(d * (J @ x - b))), float(np.linalg.norm(d * b))


def scaled_gmres(J, b, M, d, misformulated=False, **kw):
    """``kr.gmres(D J, D b, lambda t: M(t / d))``: the LinearResult's norms are the scaled ones, x solves J x = b."""
    J = sp.csr_matrix(J)
    DJ = sp.diags(d) @ J
    pre = M if misformulated else (lambda t: M(t / d))
    return kr.gmres(DJ.tocsr(), d * np.asarray(b, dtype=np.float64), pre, side="right", **kw)
