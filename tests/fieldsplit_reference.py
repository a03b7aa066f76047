"""A float64 restatement of the field-split preconditioner (fedm_amd/csrc/amg.hip) in numpy/scipy, written from the
mathematics its comments state, not from its loops: the vectors it takes and returns are in the device's vertex
numbering, like those of ``DeviceProblem.fieldsplit_apply``.

With n_eq = NS + 1 unknowns a vertex (NS species, the potential last) and J the Jacobian:

* first stage: g = Duu^-1 t_u, Duu the species part of every vertex's diagonal block;
* species sweeps (weights w_0 .. w_{m-1}): z <- zs z + w_s (g - S zs z), S = Duu^-1 J_uu, zs = w_0 in the first one
  (whose z is g itself), 1 afterwards -- so z_m = q(S) g with 1 - lambda q(lambda) = prod_i (1 - w_i lambda);
  m = 1 is block Jacobi, z_u = g;
* lower-triangular order: b_phi = t_phi - J_phi,u z_u (lagged: the iterate before the last sweep, zs z_in),
  z_phi = V-cycle(b_phi);
* upper-triangular order: z_phi = V-cycle(t_phi) first, then g = Duu^-1 (t_u - J_u,phi z_phi) and the sweeps;
* V-cycle on the multigrid hierarchy [(A_l, P_l)] (R_l = P_l^T, exact inverse of the coarsest A): V(nu, nu) with
  damped Jacobi x <- x + omega Dinv (b - A x) from x = 0, V(0, nu) without the pre-smoothing (``pre_smooth``), or
  Richardson sweeps with per-level weights w_l (the Chebyshev smoother: the pre-smoother in their order, the
  post-smoother backwards).  The composite levels of the device (products formed at set-up) are the same cycle.

``precision="emulate"`` rounds what the device stores: S to float16 (through float32, saturated), g and the
iterate between the sweeps to float32 (the last sweep's output too: it is computed in single precision), the
coupling planes J_phi,u / J_u,phi to float32, and the hierarchy's matrices to float32 when ``mg_f32`` (the
device's default, FEDM_MG_F32=1).  Sums, Duu^-1, the Jacobi diagonals and the coarse inverse stay float64.

``perturb`` names a deliberate fault for the negative controls of the tests: "omega" (the finest level's
smoothing weights x 1.01), "sweep" (one species sweep fewer), "coupling" (b_phi = t_phi; upper order: g = Duu^-1 t_u),
"lag" (the other coupling: plain where it is lagged and lagged where it is plain), "coarse" (no coarse correction on
the finest level), "neighbour" (the last stored off-diagonal entry of every row of S dropped).
"""
import numpy as np
import scipy.sparse as sp

PERTURBATIONS = ("omega", "sweep", "coupling", "lag", "coarse", "neighbour")


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _f16(a):
    return np.clip(np.asarray(a, dtype=np.float32), -65504.0, 65504.0).astype(np.float16).astype(np.float64)


def _round_matrix(M, rnd):
    M = sp.csr_matrix(M, copy=True)
    M.data = rnd(M.data)
    return M


class Multigrid:
    """The V-cycle of a host hierarchy ``levels`` = [(A_0, P_0), ..., (A_L, None)] as ``DeviceProblem.setup_multigrid``
    installs it: ``nu`` < 0 is V(0, |nu|); ``poly_weights`` [L, k]: Richardson weights per level (the polynomial
    smoother) instead of ``nu`` / ``omega``."""

    def __init__(self, levels, nu=1, omega=0.67, poly_weights=None):
        self.levels = [(sp.csr_matrix(A), None if P is None else sp.csr_matrix(P)) for A, P in levels]
        self.nu = abs(int(nu))
        self.pre_smooth = int(nu) > 0
        self.omega = float(omega)
        self.poly_weights = None if poly_weights is None else np.asarray(poly_weights, dtype=np.float64)
        self.coarse_inv = np.linalg.inv(self.levels[-1][0].toarray())

    @classmethod
    def of_problem(cls, prob, nu=2, omega=0.67, poly_degree=None, poly_fraction=8.0):
        """The cycle ``prob.setup_multigrid(nu=nu, omega=omega, poly_degree=poly_degree, ...)`` has installed."""
        from fedm_amd import amg
        levels = prob._last_hierarchy
        w = None
        if poly_degree and len(levels) > 1:
            w = amg.chebyshev_smoother_weights(levels, poly_degree, poly_fraction)
        return cls(levels, nu=nu, omega=omega, poly_weights=w)

    def _weights(self, l, perturb):
        w = (np.array(self.poly_weights[l]) if self.poly_weights is not None
             else np.full(self.nu, self.omega))
        if perturb == "omega" and l == 0:
            w = w * 1.01
        return w

    def apply(self, b, precision="float64", mg_f32=True, perturb=None):
        rnd = _f32 if (precision == "emulate" and mg_f32) else (lambda a: a)
        ops = []
        for A, P in self.levels:
            ops.append((_round_matrix(A, rnd), None if P is None else _round_matrix(P, rnd),
                        1.0 / A.diagonal()))
        return self._cycle(ops, 0, np.asarray(b, dtype=np.float64), perturb)

    def _cycle(self, ops, l, b, perturb):
        if l == len(ops) - 1:
            if perturb == "coarse" and l == 0:
                return np.zeros_like(b)
            return self.coarse_inv @ b
        A, P, dinv = ops[l]
        w = self._weights(l, perturb)
        x = np.zeros_like(b)
        if self.pre_smooth:
            for wi in w:
                x = x + wi * dinv * (b - A @ x)
        if not (perturb == "coarse" and l == 0):
            xc = self._cycle(ops, l + 1, P.T @ (b - A @ x), perturb)
            x = x + P @ xc
        for wi in w[::-1]:
            x = x + wi * dinv * (b - A @ x)
        return x


class FieldSplit:
    """M^-1 of the field split for the Jacobian ``J`` (scipy sparse, the device's numbering, n_eq = ns + 1 unknowns
    a vertex interleaved) with the cycle ``mg`` on the potential block."""

    def __init__(self, J, ns, mg, weights, order="lower", lagged=True, mg_f32=True):
        J = sp.csr_matrix(J)
        self.ns, self.neq = ns, ns + 1
        n = J.shape[0]
        self.nv = n // self.neq
        dof = np.arange(n)
        self.su = dof[dof % self.neq < ns]
        self.ph = dof[dof % self.neq == ns]
        self.Juu = J[self.su][:, self.su].tocsr()
        self.Jpu = J[self.ph][:, self.su].tocsr()
        self.Jup = J[self.su][:, self.ph].tocsr()
        blocks = np.empty((self.nv, ns, ns))
        base = np.arange(self.nv) * ns
        for r in range(ns):
            for c in range(ns):
                blocks[:, r, c] = np.asarray(self.Juu[base + r, base + c]).ravel()
        self.Dinv = np.linalg.inv(blocks)
        Dbd = sp.bsr_matrix((self.Dinv, np.arange(self.nv), np.arange(self.nv + 1)), shape=(self.nv * ns,) * 2)
        self.S = (Dbd @ self.Juu).tocsr()
        self.S.sort_indices()
        self.mg = mg
        self.weights = np.asarray(weights, dtype=np.float64)
        self.order = order
        self.lagged = bool(lagged)
        self.mg_f32 = bool(mg_f32)

    def dinv_u(self, v):
        """Duu^-1 v for a species vector v ([vertex][species])."""
        return np.einsum("vrc,vc->vr", self.Dinv, v.reshape(self.nv, self.ns)).ravel()

    def species_planes(self, precision="float64", perturb=None):
        S = _round_matrix(self.S, _f16) if precision == "emulate" else self.S.copy()
        if perturb == "neighbour":
            rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
            off = np.nonzero(S.indices // self.ns != rows // self.ns)[0]     # (indices sorted within a row)
            last = off[np.r_[rows[off][1:] != rows[off][:-1], True]]
            S.data[last] = 0.0
            S.eliminate_zeros()
        return S

    def sweeps(self, g, S, precision="float64", weights=None):
        """The species sweeps from the first stage g: (the last iterate, the one before the last sweep scaled by
        its zs -- what the lagged coupling multiplies).  One weight: block Jacobi, (g, None)."""
        w = self.weights if weights is None else weights
        rnd = _f32 if precision == "emulate" else (lambda a: a)
        if w.size == 1:
            return g, None
        g = rnd(g)
        z, prev = g, None
        for s in range(1, w.size):
            zs = w[0] if s == 1 else 1.0
            prev = zs * z
            z = rnd(prev + w[s] * (g - S @ prev))
        return z, prev

    def apply(self, t, precision="float64", perturb=None):
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        rnd = _f32 if precision == "emulate" else (lambda a: a)
        mg_f32 = self.mg_f32
        t_u, t_p = t[self.su], t[self.ph]
        S = self.species_planes(precision, perturb)
        w = self.weights[:-1] if (perturb == "sweep" and self.weights.size > 1) else self.weights
        z = np.empty_like(t)
        if self.order == "upper":
            x0 = self.mg.apply(t_p, precision, mg_f32, perturb)
            Jup = _round_matrix(self.Jup, rnd)
            g = self.dinv_u(t_u if perturb == "coupling" else t_u - Jup @ x0)
            z_u, _ = self.sweeps(g, S, precision, w)
            z[self.su], z[self.ph] = z_u, x0
            return z
        g = self.dinv_u(t_u)
        z_u, prev = self.sweeps(g, S, precision, w)
        Jpu = _round_matrix(self.Jpu, rnd)
        if perturb == "coupling":
            b = t_p.copy()
        elif (self.lagged != (perturb == "lag")) and prev is not None:
            b = t_p - Jpu @ rnd(prev)
        else:
            b = t_p - Jpu @ z_u
        z[self.su], z[self.ph] = z_u, self.mg.apply(b, precision, mg_f32, perturb)
        return z


def rel_diff(a, b, neq):
    """max over the fields of max |a - b| / max |b| (species and potential have unrelated scales)."""
    a, b = np.asarray(a).reshape(-1, neq), np.asarray(b).reshape(-1, neq)
    out = 0.0
    for f in range(neq):
        scale = np.abs(b[:, f]).max()
        if scale > 0:
            out = max(out, np.abs(a[:, f] - b[:, f]).max() / scale)
        else:
            out = max(out, np.abs(a[:, f]).max())
    return out


def sweep_polynomial(weights):
    """Coefficients (ascending) of q with z_m = q(S) g: 1 - lambda q(lambda) = prod_i (1 - w_i lambda)."""
    from numpy.polynomial import polynomial as npoly
    p = np.array([1.0])
    for wi in weights:
        p = npoly.polymul(p, [1.0, -wi])
    r = npoly.polysub([1.0], p)        # lambda q(lambda)
    assert abs(r[0]) < 1e-15
    return r[1:]


def balanced_rhs(J, ns, rng):
    """t = J x for a random x: a vector of the kind the Krylov method hands the preconditioner, in which every block
    of J leaves its mark (a t of unit entries would not -- the species rows of J are some 10^15 times the potential
    block's, so J_phi,u z_u would vanish beside t_phi).  x_u ~ N(0, 1); x_phi scaled so that K x_phi and J_phi,u x_u
    are of one size."""
    J = sp.csr_matrix(J)
    neq = ns + 1
    dof = np.arange(J.shape[0])
    su, ph = dof[dof % neq < ns], dof[dof % neq == ns]
    x = rng.standard_normal(J.shape[0])
    cpl = np.abs(J[ph][:, su] @ x[su]).max()
    pot = np.abs(J[ph][:, ph] @ x[ph]).max()
    x[ph] *= cpl / pot if pot > 0 and cpl > 0 else 1.0
    return J @ x
