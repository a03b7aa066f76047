"""numpy / scipy restatement of the photoionisation source (helper module of the photoionisation tests).

    S_ph = sum_m c_m y_m,      (-lap + kappa_m^2) y_m = efficiency * R,

weak form ``int (grad y . grad v + kappa^2 y v) w dx = int efficiency R v w dx`` with ``w = x[0]`` for an axisymmetric
model and 1 otherwise; ``y = 0`` on the vertices of the facets with a listed tag, zero flux elsewhere.  Written from the
weak form, independently of fedm_amd/photo.py and csrc/photo.hip: the geometry, the cell fields and the densities are
``oracle.forms.LFAModel``'s own (``detJ``, ``G``, ``xc``, ``cell_fields``, ``_dens``, the reactions' term sums), the
quadrature rule is the oracle's ``triangle_rule(qdeg_source)``, the solves are ``spsolve``.

tests/test_photoionization_reference.py pins this module on a manufactured solution; tests/test_gpu_photoionization.py
holds the device to it.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.lagrange import p1_basis
from oracle.quadrature import triangle_rule


def perturbed(U0, seed):
    """The perturbation of tests/test_gpu_parity.py (``_perturbed``): densities and potential off their smooth start."""
    rng = np.random.default_rng(seed)
    U = U0.copy()
    U[:, 0] += rng.normal(0, 0.05, U.shape[0])
    U[:, 1] += rng.normal(0, 0.3, U.shape[0])
    U[:, 2] += rng.normal(0, 20.0, U.shape[0])
    return U


def _points(om):
    """[(phi[3], W[cell])]: the basis at the model's quadrature points and weight * |det J| * w there."""
    xq, wq = triangle_rule(om.qdeg_source)
    w_nodes = om.xc[:, :, 0] if om.axisymmetric else np.ones(om.xc.shape[:2])
    out = []
    for xi, w in zip(xq, wq):
        phi = p1_basis(xi[None, :])[0]
        out.append((phi, w * om.detJ * (w_nodes @ phi)))
    return out


def _scatter_matrix(om, elem):
    c = om.mesh.cells.astype(np.int64)
    A = sp.csr_matrix((om.mesh.nv, om.mesh.nv))
    for a in range(3):
        for b in range(3):
            A = A + sp.coo_matrix((elem[:, a, b], (c[:, a], c[:, b])), shape=A.shape).tocsr()
    return A.tocsr()


def matrices(om):
    """(K_w, M_w): ``int w grad(phi_a).grad(phi_b)`` and ``int w phi_a phi_b`` by the model's quadrature rule."""
    nc = om.mesh.nc
    Ke, Me = np.zeros((nc, 3, 3)), np.zeros((nc, 3, 3))
    for phi, W in _points(om):
        for a in range(3):
            for b in range(3):
                Ke[:, a, b] += W * (om.G[:, a, 0] * om.G[:, b, 0] + om.G[:, a, 1] * om.G[:, b, 1])
                Me[:, a, b] += W * phi[a] * phi[b]
    return _scatter_matrix(om, Ke), _scatter_matrix(om, Me)


def rate_at_points(om, U, reactions):
    """R[point][cell] = sum_j k_j(|E|) prod_i n_i^P_ji: k_j once per cell at the cell's |E|, the densities at the points."""
    Uc, _, Em = om.cell_fields(U)
    out = []
    for phi, _ in _points(om):
        n = [om._dens(Uc[:, :, s] @ phi)[0] for s in range(om.ns)]
        R = np.zeros(om.mesh.nc)
        for j in reactions:
            k, P, _ = om.reactions[j]
            prod = np.ones(om.mesh.nc)
            for i in range(om.ns):
                if P[i]:
                    prod = prod * n[i] ** P[i]
            R = R + k(Em)[0] * prod
        out.append(R)
    return out


def load_vector(om, rate, efficiency):
    """g_a = int efficiency R phi_a w; ``rate``: R[point][cell] (rate_at_points) or a number."""
    g = np.zeros(om.mesh.nv)
    for q, (phi, W) in enumerate(_points(om)):
        R = rate[q] if not np.isscalar(rate) else rate
        for a in range(3):
            np.add.at(g, om.mesh.cells[:, a], W * efficiency * R * phi[a])
    return g


def zero_mask(om, zero_tags):
    """The vertices of the facets whose tag is listed; facet i of a cell lies opposite its vertex i."""
    mask = np.zeros(om.mesh.nv, dtype=bool)
    if om.facet_tags is None:
        return mask
    for cell, i in zip(*np.nonzero(np.isin(om.facet_tags, list(zero_tags)))):
        for a in range(3):
            if a != i:
                mask[om.mesh.cells[cell, a]] = True
    return mask


def eliminate(A, mask):
    """Rows and columns of the masked vertices out, unit diagonal in (the values there are 0: nothing moves right)."""
    A = A.tolil(copy=True)
    idx = np.nonzero(mask)[0]
    A[idx, :] = 0.0
    A[:, idx] = 0.0
    A[idx, idx] = 1.0
    return A.tocsr()


def operators(om, kappa, zero_tags):
    K, M = matrices(om)
    mask = zero_mask(om, zero_tags)
    return [eliminate(K + k ** 2 * M, mask) for k in kappa], mask


def solve(A, g, mask):
    b = np.where(mask, 0.0, g)
    return spla.spsolve(A.tocsc(), b)


def table(om, y, c):
    """ext[cell][a] = sum_m c_m y_m[vertex a of the cell]."""
    S = sum(cm * ym for cm, ym in zip(c, y))
    return S[om.mesh.cells]


def reference(om, U_old, reactions, efficiency, c, kappa, zero_tags):
    """Everything of one update: dict(g, mask, A, y, table)."""
    A, mask = operators(om, kappa, zero_tags)
    g = np.where(mask, 0.0, load_vector(om, rate_at_points(om, U_old, reactions), efficiency))
    y = np.array([solve(Am, g, mask) for Am in A])
    return dict(g=g, mask=mask, A=A, y=y, table=table(om, y, c))


def exact_strip(z, d, kappa, rhs):
    """(-y'' + kappa^2 y = rhs on (0, d), y(0) = y(d) = 0."""
    return rhs / kappa ** 2 * (1.0 - np.cosh(kappa * (z - 0.5 * d)) / np.cosh(0.5 * kappa * d))


def mean_edge_length(coords, cells):
    e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    return float(np.linalg.norm(coords[e[:, 0]] - coords[e[:, 1]], axis=1).mean())
