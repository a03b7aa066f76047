"""numpy restatement of the discharge diagnostics (helper module of the diagnostics tests).

Written from the formulae of include/fedm_hip.h (fedm_diagnostics), independently of csrc/diag.hip, on the oracle's
model objects: geometry (``detJ``, ``G``, ``xc``, ``rnod``), cell fields, densities and coefficients are
``oracle.forms.LFAModel``'s own, the quadrature rule is the oracle's ``triangle_rule(qdeg_source)``.

    W_q      = w_q |det J| 2 pi w(x_q)                      w = r (axisymmetric) or 1/(2 pi)
    N_s      = sum_cells sum_q W_q om n_s(x_q)
    R_Phi,i  = sum_cells sum_q W_q (grad Phi . grad phi_i - (e/eps0) sum_s Z_s n_s phi_i),   q_g = sum_(i in g) R_Phi,i
    I_psi    = sum_s Z_s sum_cells sum_q W_q om Gamma_s(x_q) . (-grad psi)
    Gamma_s  = n_s (-D_s grad u_s + Z_s mu_s E)   or, linear representation,   -D_s grad u_s + Z_s mu_s E u_s

``om`` is 1, or with an ``owned`` mask the sum of the owned vertices' basis functions at the point (a rank's share).
Every sum comes back as ``Sum(value, abs)``: ``math.fsum`` of its terms and the sum of their magnitudes.  A term is
one addend of the formula at one quadrature point: for N_s the product ``W om n_s``; for a Poisson row the gradient
part ``W grad Phi . grad phi_i`` and each species' charge part ``-W (e/eps0) Z_s n_s phi_i`` separately; for the
current each species' diffusive part and its drift part separately.  (An implementation forms these addends in
floating point before it adds them, so their magnitudes, not the magnitude of their difference, bound its rounding.)
Every maximum comes back as ``Max(value, index, unique, centroid)``: the lowest index that attains it, whether it is
the only one, and for cells the centroid ``(x_0 + x_1 + x_2) / 3``; value 0 and index -1 where nothing is eligible.

tests/test_diagnostics_reference.py pins this module on closed forms; tests/test_gpu_diagnostics.py holds the device
to it.
"""
import math
from collections import namedtuple

import numpy as np

from oracle.forms import DRIFT_DIFFUSION_REACTION, REACTION, elementary_charge, epsilon_0
from oracle.lagrange import p1_basis
from oracle.quadrature import triangle_rule

Sum = namedtuple("Sum", "value abs")
Max = namedtuple("Max", "value index unique centroid")


def _sum(*arrays):
    flat = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]) if arrays else np.zeros(0)
    return Sum(math.fsum(flat.tolist()), math.fsum(np.abs(flat).tolist()))


def _max(values, eligible, centroids=None):
    idx = np.nonzero(eligible)[0]
    if idx.size == 0:
        return Max(0.0, -1, True, None if centroids is None else (0.0, 0.0))
    v = values[idx]
    top = v.max()
    at = idx[v == top]
    c = None if centroids is None else (float(centroids[at[0], 0]), float(centroids[at[0], 1]))
    return Max(float(top), int(at[0]), at.size == 1, c)


def centroids(om):
    x = om.xc
    return (x[:, 0] + x[:, 1] + x[:, 2]) / 3.0


def points(om, owned=None):
    """[(phi[3], W[cell], om[cell])] at the model's quadrature points."""
    xq, wq = triangle_rule(om.qdeg_source)
    own = None if owned is None else np.asarray(owned, dtype=bool)[om.mesh.cells]      # (Nc, 3)
    out = []
    for xi, w in zip(xq, wq):
        phi = p1_basis(xi[None, :])[0]
        W = w * om.detJ * (2.0 * np.pi) * (om.rnod @ phi)
        weight = np.ones(om.mesh.nc) if own is None else np.where(own.all(axis=1), 1.0, (own * phi[None, :]).sum(axis=1))
        out.append((phi, W, weight))
    return out


def reference(om, U, window=None, psi=None, group=None, n_groups=0, owned=None):
    """dict(species=[Sum], groups=[Sum], current=Sum, field=Max, window=Max, nodal=[Max]) of the state U[nv, neq]."""
    U = np.asarray(U, dtype=np.float64)
    nc, ns = om.mesh.nc, om.ns
    cells = om.mesh.cells
    Uc, E, Em = om.cell_fields(U)
    own_v = np.ones(om.mesh.nv, dtype=bool) if owned is None else np.asarray(owned, dtype=bool)
    pts = points(om, owned)
    dens = [[om._dens(Uc[:, :, s] @ phi)[0] for s in range(ns)] for phi, _, _ in pts]

    species = [_sum(*[W * wt * dens[q][s] for q, (_, W, wt) in enumerate(pts)]) for s in range(ns)]

    # -- induced current ---------------------------------------------------------------------------------------------
    cur_terms = []
    if psi is not None:
        mgpsi = -np.einsum("ca,cad->cd", np.asarray(psi, dtype=np.float64)[cells], om.G)          # -grad(psi)
        for s in range(ns):
            if om.eq_type[s] == REACTION:
                continue
            gradu = np.einsum("ca,cad->cd", Uc[:, :, s], om.G)
            Dv = om.D[s](Em)[0]
            drift = None
            if om.eq_type[s] == DRIFT_DIFFUSION_REACTION:
                if om.drift_w[s] is not None:
                    drift = np.broadcast_to(np.asarray(om.drift_w[s], dtype=np.float64)[None, :], (nc, 2))
                elif om.poisson:
                    drift = (om.Z[s] * om.mu[s](Em)[0])[:, None] * E
            dif_p = np.einsum("cd,cd->c", -Dv[:, None] * gradu, mgpsi)
            dri_p = np.zeros(nc) if drift is None else np.einsum("cd,cd->c", drift, mgpsi)
            for q, (_, W, wt) in enumerate(pts):
                n = dens[q][s]
                cur_terms.append(om.Z[s] * W * wt * dif_p * (n if om.log else 1.0))
                cur_terms.append(om.Z[s] * W * wt * dri_p * n)
    current = _sum(*cur_terms)

    # -- Poisson rows over the vertex groups ------------------------------------------------------------------------
    groups = []
    if n_groups:
        assert om.poisson
        grp = np.asarray(group)
        gP = -E
        coe = elementary_charge / epsilon_0
        for g in range(1, n_groups + 1):
            terms = []
            for a in range(3):
                hit = (grp[cells[:, a]] == g) & own_v[cells[:, a]]
                if not hit.any():
                    continue
                gG = np.einsum("cd,cd->c", gP, om.G[:, a])
                for q, (phi, W, _) in enumerate(pts):
                    terms.append((W * gG)[hit])
                    for s in range(ns):
                        terms.append((-W * coe * om.Z[s] * dens[q][s] * phi[a])[hit])
            groups.append(_sum(*terms))

    # -- maxima ------------------------------------------------------------------------------------------------------
    cen = centroids(om)
    if om.poisson:
        eligible = own_v[cells].any(axis=1)
        field = _max(Em, eligible, cen)
        inside = eligible.copy()
        if window is not None:
            r_lo, r_hi, z_lo, z_hi = window
            inside &= (cen[:, 0] >= r_lo) & (cen[:, 0] <= r_hi) & (cen[:, 1] >= z_lo) & (cen[:, 1] <= z_hi)
        win = _max(Em, inside, cen)
    else:
        field = win = Max(0.0, -1, True, (0.0, 0.0))
    nodal = [_max(U[:, s], own_v) for s in range(ns)]
    return dict(species=species, groups=groups, current=current, field=field, window=win, nodal=nodal)


def combine_sums(shares):
    """The ranks' shares of one sum: Sum(fsum of the values, sum of the magnitudes' sums)."""
    return Sum(math.fsum(s.value for s in shares), math.fsum(s.abs for s in shares))


def combine_maxima(shares, to_global):
    """The ranks' maxima of one quantity: the largest value wins, ties go to the lower global index.
    ``to_global[rank]`` maps a local index.  Returns (value, global index)."""
    best = (0.0, -1)
    for rank, m in enumerate(shares):
        if m.index < 0:
            continue
        g = int(to_global[rank][m.index])
        if best[1] < 0 or m.value > best[0] or (m.value == best[0] and g < best[1]):
            best = (m.value, g)
    return best
