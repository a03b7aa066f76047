"""Host set-up of the photoionisation source (three-term Helmholtz approximation, Bourdon et al. 2007).

``S_ph = sum_m c_m y_m`` with ``(-lap + kappa_m^2) y_m = efficiency * R``, ``R`` the rate of the model's designated
ionisation reactions.  The operators ``K_w + kappa_m^2 M_w`` do not change during a run: they are assembled here once
per mesh (numpy/scipy, cold path), their multigrid hierarchies built with :mod:`fedm_amd.amg`, and handed to the
device (``fedm_photo_setup``), where every update -- load vector, conjugate gradients, source tables -- runs
(csrc/photo.hip).  ``w = x[0]`` for an axisymmetric model and 1 otherwise, the convention of
``weak_form_Poisson_equation`` without its ``2 pi``.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import scipy.sparse as sp

from . import _lib, quadrature


@dataclass
class Photoionization:
    """Photoionisation of a :class:`fedm_amd.device.Model` (its ``photoionization`` field).

    ``reactions``: indices into the model's reactions whose summed rate is the ionisation rate ``R``;
    ``c`` [1/m^2] and ``kappa`` [1/m]: the Helmholtz terms (at most 4); ``targets``: the species whose balance
    equations receive ``S_ph`` (through their degree-1 source tables); ``zero_tags``: boundary tags on whose vertices
    ``y_m = 0`` (zero flux elsewhere).  ``rtol``, ``max_it``: of the conjugate gradients, ``|r| <= rtol |b|``.
    ``multigrid``: smoothed-aggregation V(nu,nu) cycles as preconditioner (Jacobi alone when False, or when the mesh is
    smaller than ``max_coarse`` vertices)."""
    reactions: Sequence[int]
    efficiency: float
    c: Sequence[float]
    kappa: Sequence[float]
    targets: Sequence[int]
    zero_tags: Sequence[int] = ()
    rtol: float = 1e-6
    max_it: int = 500
    multigrid: bool = True
    max_coarse: int = 600
    nu: int = 1
    omega: float = 0.67
    theta: float = 0.08

    def check(self, model):
        """ValueError for what the device would refuse (and what only the host can see)."""
        if not 1 <= len(self.c) <= _lib.PHOTO_MAX_TERMS or len(self.c) != len(self.kappa):
            raise ValueError(f"Photoionization: 1 to {_lib.PHOTO_MAX_TERMS} Helmholtz terms, one c and one kappa each")
        if any(not (k > 0.0) or not np.isfinite(k) for k in self.kappa):
            raise ValueError("Photoionization: every kappa must be positive and finite")
        if not self.reactions or any(not 0 <= int(j) < len(model.reactions) for j in self.reactions):
            raise ValueError(f"Photoionization: reactions must index the model's {len(model.reactions)} reactions")
        if not self.targets or any(not 0 <= int(s) < model.n_species for s in self.targets):
            raise ValueError(f"Photoionization: targets must be species 0..{model.n_species - 1}")
        if any(not 1 <= int(t) <= len(model.bc_kind) for t in self.zero_tags):
            raise ValueError(f"Photoionization: zero_tags must be boundary tags 1..{len(model.bc_kind)}")
        if not self.rtol > 0.0:
            raise ValueError("Photoionization: rtol must be positive")

    def to_c(self):
        d = _lib.PhotoDesc()
        d.n_terms, d.n_src = len(self.c), len(self.reactions)
        for m in range(len(self.c)):
            d.c[m], d.kappa[m] = float(self.c[m]), float(self.kappa[m])
        d.efficiency = float(self.efficiency)
        for k, j in enumerate(self.reactions):
            d.src_reaction[k] = int(j)
        d.target_species_mask = sum(1 << int(s) for s in set(self.targets))
        d.zero_tag_mask = sum(1 << (int(t) - 1) for t in set(self.zero_tags))
        return d


def helmholtz_matrices(coords, cells, axisymmetric, quadrature_degree):
    """``(K_w, M_w)`` of the P1 space: ``int w grad(phi_a).grad(phi_b)`` and ``int w phi_a phi_b`` at the points of the
    model's quadrature rule (``w`` is linear: the stiffness is exact; the mass is the consistent one)."""
    x = coords[cells]
    d1, d2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    det = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
    G = np.stack([np.stack([x[:, 1, 1] - x[:, 2, 1], x[:, 2, 0] - x[:, 1, 0]], axis=1),
                  np.stack([x[:, 2, 1] - x[:, 0, 1], x[:, 0, 0] - x[:, 2, 0]], axis=1),
                  np.stack([x[:, 0, 1] - x[:, 1, 1], x[:, 1, 0] - x[:, 0, 0]], axis=1)], axis=1) / det[:, None, None]
    w_nodes = x[:, :, 0] if axisymmetric else np.ones(x.shape[:2])
    xq, wq = quadrature.triangle(quadrature_degree)
    phi = np.stack([1.0 - xq[:, 0] - xq[:, 1], xq[:, 0], xq[:, 1]], axis=1)          # [point][a]
    W = np.abs(det)[:, None] * wq[None, :] * (w_nodes @ phi.T)                         # [cell][point]
    Ke = np.einsum("cad,cbd->cab", G, G) * W.sum(axis=1)[:, None, None]
    Me = np.einsum("cq,qa,qb->cab", W, phi, phi)
    c = cells.astype(np.int64)
    rows = np.broadcast_to(c[:, :, None], Ke.shape).ravel()
    cols = np.broadcast_to(c[:, None, :], Ke.shape).ravel()
    n = coords.shape[0]
    build = lambda e: sp.coo_matrix((e.ravel(), (rows, cols)), shape=(n, n)).tocsr()
    return build(Ke), build(Me)


def zero_vertices(cells, facet_tags, zero_tags, n_vertices):
    """Boolean mask of the vertices of the facets whose tag is listed (facet i lies opposite vertex i)."""
    mask = np.zeros(n_vertices, dtype=bool)
    if facet_tags is None or not len(zero_tags):
        return mask
    tags = np.asarray(facet_tags).reshape(-1, 3)
    hit = np.isin(tags, np.asarray(list(zero_tags)))
    for i in range(3):
        sel = hit[:, i]
        mask[cells[sel, (i + 1) % 3]] = True
        mask[cells[sel, (i + 2) % 3]] = True
    return mask


def eliminate(A, fixed):
    """Rows and columns of the fixed vertices replaced by unit rows (symmetric elimination; the right-hand side is 0
    there, so nothing moves to it)."""
    keep = sp.diags((~fixed).astype(np.float64))
    out = (keep @ A @ keep + sp.diags(fixed.astype(np.float64))).tocsr()
    out = (0.5 * (out + out.T)).tocsr()          # (a, b) and (b, a) were summed in different orders: exactly symmetric
    out.eliminate_zeros()
    out.sort_indices()
    return out


def install(lib, handle, photo: Photoionization, coords, cells, facet_tags, axisymmetric, quadrature_degree):
    """Assemble the terms' operators in the numbering given (the device's), build their hierarchies and call
    ``fedm_photo_setup``.  Returns the level sizes per term."""
    from . import amg
    K, M = helmholtz_matrices(coords, cells, axisymmetric, quadrature_degree)
    fixed = zero_vertices(cells, facet_tags, photo.zero_tags, coords.shape[0])
    terms = (_lib.PhotoHierarchy * len(photo.c))()
    keep, sizes = [], []
    for m, kappa in enumerate(photo.kappa):
        A = eliminate(K + float(kappa) ** 2 * M, fixed)
        levels = [(A, None)]
        if photo.multigrid:
            levels = amg.build_hierarchy(A, theta=photo.theta, max_coarse=photo.max_coarse, fixed=fixed, coords=coords)
        terms[m], held = amg.pack_hierarchy(levels, photo.nu, photo.omega)
        keep.append(held)
        sizes.append([a.shape[0] for a, _ in levels])
    desc = photo.to_c()
    rc = lib.fedm_photo_setup(handle, C.byref(desc), terms)
    if rc != 0:
        raise RuntimeError(f"fedm_photo_setup failed ({rc}): {_lib.last_error()}")
    return sizes
