"""A float64 restatement of the solvers of fedm_amd/csrc (``gmres()`` in krylov.cpp, ``fedm_newton_solve`` in
newton.cpp) in numpy/scipy, written from the algorithms DESIGN.md section 4 names, not from the driver's loops:
restarted GMRES(m), flexible with the preconditioner on the right (z_j = M^-1 v_j kept, x += Z y, stopping test on
the true residual's recurrence) or with the preconditioner on the left (M^-1 J x = M^-1 b, stopping test on the
preconditioned residual), and the Newton loop with PETSc's ``newtonls`` / ``basic`` tests.

It is a predictor, not a bit-level twin of the device: modified Gram-Schmidt with full re-orthogonalisation (two passes
every step, norms taken explicitly) where the device runs classical Gram-Schmidt in one pass and forms
``|w - V h|^2 = ww - |h|^2`` by subtraction.  It tells, without a GPU, roughly how many steps an input needs -- so that
the inputs of tests/test_gpu_krylov.py can be chosen to land on a path of the driver -- and what a correct solve's true
residual is.  The preconditioner is a callable ``M(t) -> z``; ``fieldsplit_reference.FieldSplit.apply`` plugs in,
plain or with ``precision="emulate"``.

``fault`` names a deliberate fault for the negative controls (FAULTS): "drop_last_column" (the last column of H is left
out of the back substitution: y_k = 0), "skip_rotation" (the first Givens rotation is not applied to the later columns),
"no_accumulate" (x = Z y in every cycle instead of x += Z y), "stale_y" (from the second cycle on the y of the cycle
before is used again).  A faulty solve still reports the recurrence's norm: it 'converges', with a wrong x.
"""
import numpy as np

FAULTS = ("drop_last_column", "skip_rotation", "no_accumulate", "stale_y")
CONVERGED, DIVERGED_MAX_IT, DIVERGED_NAN, DIVERGED_LINEAR = 0, 1, 2, 3     # include/fedm_hip.h FEDM_DIVERGED_*


class LinearResult:
    def __init__(self, x, its, rnorm, code, cycles, history):
        self.x, self.its, self.rnorm, self.code, self.cycles, self.history = x, its, rnorm, code, cycles, history

    def __repr__(self):
        return f"LinearResult(its={self.its}, rnorm={self.rnorm:.3e}, code={self.code}, cycles={self.cycles})"


def gmres(J, b, M=None, side="right", restart=30, rtol=1e-5, atol=1e-50, max_it=10000, fault=None):
    """GMRES(restart) on J x = b from x = 0.  ``side="right"``: flexible, right-preconditioned; stops when the
    residual norm of J x = b falls to max(rtol |b|, atol).  ``side="left"``: on M^-1 J x = M^-1 b with that system's
    residual and max(rtol |M^-1 b|, atol).  Returns a LinearResult: x, the number of Krylov steps, the norm the
    recurrence reports (after ``max_it`` steps without convergence: the true norm of that system's residual, and code
    DIVERGED_LINEAR), the cycles that ran a step, and the recurrence's norm after every step."""
    assert side in ("right", "left") and fault in (None,) + FAULTS
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    M = M if M is not None else (lambda t: t)
    if side == "left":
        op = lambda v: M(J @ v)
        rhs = M(b)
    else:
        op = lambda v: J @ v
        rhs = b
    x = np.zeros(n)
    m = int(restart)
    its = cycles = 0
    history = []
    r0 = float(np.linalg.norm(rhs))
    if not np.isfinite(r0):
        return LinearResult(x, 0, r0, DIVERGED_NAN, 0, history)
    tol = max(rtol * r0, atol)
    rnorm = r0
    y_prev = None
    while True:
        r = rhs - op(x) if its else rhs.copy()
        beta = float(np.linalg.norm(r))
        rnorm = beta
        if beta <= tol or its >= max_it:
            break
        V = np.zeros((m + 1, n))
        Z = np.zeros((m, n))
        H = np.zeros((m + 1, m))
        R = np.zeros((m + 1, m))          # H after the rotations
        cs, sn = np.zeros(m), np.zeros(m)
        g = np.zeros(m + 1)
        g[0] = beta
        V[0] = r / beta
        k = 0
        done = False
        while k < m and its < max_it:
            if side == "right":
                Z[k] = M(V[k])
                w = J @ Z[k]
            else:
                Z[k] = V[k]
                w = op(V[k])
            for _ in range(2):                          # modified Gram-Schmidt, twice
                for i in range(k + 1):
                    h = float(V[i] @ w)
                    H[i, k] += h
                    w = w - h * V[i]
            hn = float(np.linalg.norm(w))
            H[k + 1, k] = hn
            if not np.isfinite(hn):
                return LinearResult(x, its, hn, DIVERGED_NAN, cycles, history)
            if hn > 0.0:
                V[k + 1] = w / hn
            col = H[:k + 2, k].copy()
            for i in range(k):
                if fault == "skip_rotation" and i == 0:
                    continue
                t = cs[i] * col[i] + sn[i] * col[i + 1]
                col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
                col[i] = t
            d = float(np.hypot(col[k], col[k + 1]))
            cs[k], sn[k] = (col[k] / d, col[k + 1] / d) if d > 0.0 else (1.0, 0.0)
            col[k], col[k + 1] = d, 0.0
            R[:k + 2, k] = col
            g[k + 1] = -sn[k] * g[k]
            g[k] = cs[k] * g[k]
            its += 1
            k += 1
            rnorm = abs(g[k])
            history.append(rnorm)
            if rnorm <= tol or hn == 0.0:
                done = True
                break
        y = np.zeros(k)
        kk = k - 1 if (fault == "drop_last_column" and k > 1) else k
        for i in range(kk - 1, -1, -1):
            y[i] = (g[i] - R[i, i + 1:kk] @ y[i + 1:kk]) / R[i, i]
        if fault == "stale_y" and y_prev is not None:
            y = np.resize(y_prev, k) if y_prev.size >= k else np.r_[y_prev, np.zeros(k - y_prev.size)]
        y_prev = y.copy()
        if k:
            cycles += 1
            x = (Z[:k].T @ y) if (fault == "no_accumulate") else x + Z[:k].T @ y
        if done:
            break
        if its >= max_it:
            rnorm = float(np.linalg.norm(rhs - op(x)))
            break
    return LinearResult(x, its, rnorm, CONVERGED if rnorm <= tol else DIVERGED_LINEAR, cycles, history)


def block_jacobi(J, neq):
    """M^-1 of point-block Jacobi: the inverse of every vertex's neq x neq diagonal block of J (what the device falls
    to, on the left, without a multigrid hierarchy)."""
    import scipy.sparse as sp
    J = sp.csr_matrix(J)
    nv = J.shape[0] // neq
    blocks = np.empty((nv, neq, neq))
    base = np.arange(nv) * neq
    for r in range(neq):
        for c in range(neq):
            blocks[:, r, c] = np.asarray(J[base + r, base + c]).ravel()
    inv = np.linalg.inv(blocks)
    return lambda t: np.einsum("vrc,vc->vr", inv, np.asarray(t).reshape(nv, neq)).ravel()


class NewtonResult:
    def __init__(self, u, its, code, linear_its, fnorms, snorms):
        self.u, self.its, self.code, self.linear_its, self.fnorms, self.snorms = u, its, code, linear_its, fnorms, snorms


def newton(residual_jacobian, u0, rtol=1e-9, atol=1e-10, stol=1e-16, max_it=50, linear_solve=None):
    """PETSc ``newtonls`` with the ``basic`` line search (full steps) as DESIGN.md section 4 states its tests: at
    iteration 0 only |F| < atol; afterwards |F| < atol, |F| <= rtol |F0| or |delta| < stol |u| (delta the update
    just made, u the state after it); not converged at ``max_it`` -> DIVERGED_MAX_IT; a non-finite |F| ->
    DIVERGED_NAN; a linear solve that fails -> DIVERGED_LINEAR.  ``residual_jacobian(u) -> (F, J)``;
    ``linear_solve(J, b) -> LinearResult`` (default: a direct solve).  ``snorms[i]`` is |delta| / |u| of update i + 1."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    if linear_solve is None:
        linear_solve = lambda J, b: LinearResult(spla.spsolve(sp.csc_matrix(J), b), 0, 0.0, CONVERGED, 0, [])
    u = np.array(u0, dtype=np.float64)
    it = lin = 0
    fnorms, snorms = [], []
    snorm = xnorm = 0.0
    while True:
        F, J = residual_jacobian(u)
        fnorm = float(np.linalg.norm(F))
        fnorms.append(fnorm)
        if not np.isfinite(fnorm):
            return NewtonResult(u, it, DIVERGED_NAN, lin, fnorms, snorms)
        if it == 0:
            done = fnorm < atol
        else:
            done = fnorm < atol or fnorm <= rtol * fnorms[0] or snorm < stol * xnorm
        if done:
            return NewtonResult(u, it, CONVERGED, lin, fnorms, snorms)
        if it >= max_it:
            return NewtonResult(u, it, DIVERGED_MAX_IT, lin, fnorms, snorms)
        res = linear_solve(J, -F)
        lin += res.its
        if res.code != CONVERGED:
            return NewtonResult(u, it, res.code if res.code == DIVERGED_NAN else DIVERGED_LINEAR, lin, fnorms, snorms)
        u = u + res.x
        snorm, xnorm = float(np.linalg.norm(res.x)), float(np.linalg.norm(u))
        snorms.append(snorm / xnorm if xnorm > 0 else np.inf)
        it += 1
