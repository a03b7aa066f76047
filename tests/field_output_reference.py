"""numpy restatement of the field output (helper module of the field-output tests).

Written from the table of include/fedm_hip.h (fedm_fields), independently of csrc/fields.hip, on the oracle's model
objects: geometry (``detJ``, ``G``), cell fields, densities and coefficients are ``oracle.forms.LFAModel``'s own, the
quadrature rule is the oracle's ``triangle_rule(qdeg_source)``.

    STATE e      u_e(v)                         DENSITY s   exp(u_s(v)), linear representation u_s(v)
    CHARGE       e sum_s Z_s n_s(v)
    E_R, E_Z     the cell-constant -dPhi/dr, -dPhi/dz                       projected
    E_NORM       the cell-constant |E|                                      projected
    RATE j       k_j(|E|) prod_i n_i(x_q)^p_ji                              projected
    FLUX_R/Z s   n_s (-D_s grad u_s + w_s), linear -D_s grad u_s + w_s u_s  projected
                 w_s = drift_w, or Z_s mu_s E (with a Poisson equation); 0 for 'reaction' species

Projection in the plain measure dx (no r, no 2 pi):

    b_v = sum_(c with v) sum_q w_q |det J_c| f(x_q) phi_v(x_q),   m_v = sum_(c with v) |det J_c| / 6,
    lumped X = b / m,   consistent M X = b with the P1 mass matrix (spsolve).

A projected kind comes back as ``Projected(b, abs, m)``: ``b_v`` as the ``math.fsum`` of its terms, ``abs`` the sum of
their magnitudes, ``m`` the lumped mass.  A term is one addend at one quadrature point of one cell, ``w_q |det J| t
phi_v``, where the ``t`` are the addends an implementation has to form in floating point before it adds them (their
magnitudes, not the magnitude of their sum, bound its rounding -- diagnostics_reference.py's rule).  A gradient
component is three addends, one per corner (``-Phi_a dphi_a/dr``: where the potential does not depend on r they
cancel to exactly 0 in one order of evaluation and to a rounding residue in another), so E_R and E_Z have three per
point; a flux has its diffusive part's three (``-D u_a dphi_a n``) and its drift part's three (or the one of a
prescribed drift); a rate is one.  E_NORM is one addend, |E|, but it is formed from the two gradient components:
``abs`` adds the magnitudes of THEIR addends, which bound |E| and its rounding (``cell_magnitudes``).  Pointwise kinds come
back as ``Pointwise(value, abs)``, ``abs`` the sum of the magnitudes of the addends of the value (CHARGE: e |Z_s| n_s).

tests/test_field_output_reference.py pins this module on closed forms; tests/test_gpu_field_output.py holds the device
to it.
"""
import math
from collections import namedtuple

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.forms import DRIFT_DIFFUSION_REACTION, REACTION, elementary_charge
from oracle.lagrange import p1_basis
from oracle.quadrature import triangle_rule

Projected = namedtuple("Projected", "b abs m")
Pointwise = namedtuple("Pointwise", "value abs")

KINDS = ("state", "density", "charge", "e_r", "e_z", "e_norm", "rate", "flux_r", "flux_z")
PROJECTED = ("e_r", "e_z", "e_norm", "rate", "flux_r", "flux_z")


def parse(name):
    """(kind, index) of a name such as "E_norm", "rate:0", "flux_z:1"."""
    head, _, tail = name.partition(":")
    kind = head.lower()
    assert kind in KINDS, name
    return kind, int(tail) if tail else 0


def points(om):
    """[(phi[3], W[cell])]: the basis at the model's quadrature points and w_q |det J| there (the plain measure)."""
    xq, wq = triangle_rule(om.qdeg_source)
    return [(p1_basis(xi[None, :])[0], w * om.detJ) for xi, w in zip(xq, wq)]


def lumped_mass(om):
    """m_v = sum over the vertex's cells of |det J| / 6 (fsum)."""
    return _vertex_fsum(om, [[om.detJ / 6.0] * 3])[0]


def mass_matrix(om):
    """The consistent P1 mass matrix of the plain measure: |det J| / 24 (1 + delta_ab) per cell."""
    c = om.mesh.cells.astype(np.int64)
    M = sp.csr_matrix((om.mesh.nv, om.mesh.nv))
    for a in range(3):
        for b in range(3):
            M = M + sp.coo_matrix((om.detJ * (2.0 if a == b else 1.0) / 24.0, (c[:, a], c[:, b])), shape=M.shape).tocsr()
    return M.tocsr()


def _vertex_fsum(om, term_sets):
    """``term_sets``: a list of [t_0[cell], t_1[cell], t_2[cell]] (the corner entries of one addend).  Returns
    (fsum per vertex, sum of magnitudes per vertex)."""
    nv, cells = om.mesh.nv, om.mesh.cells
    lists = [[] for _ in range(nv)]
    for corner in term_sets:
        for a in range(3):
            t = np.broadcast_to(np.asarray(corner[a], dtype=np.float64), (om.mesh.nc,))
            for v, x in zip(cells[:, a].tolist(), t.tolist()):
                lists[v].append(x)
    return (np.array([math.fsum(l) for l in lists]), np.array([math.fsum(abs(x) for x in l) for l in lists]))


def cell_integrands(om, U, kind, index):
    """The addends of f at the quadrature points: a list over the points of lists of arrays [cell] (one array per
    addend of the formula; their sum is f(x_q))."""
    U = np.asarray(U, dtype=np.float64)
    nc = om.mesh.nc
    Uc, E, Em = om.cell_fields(U)
    pts = points(om)
    Phi = Uc[:, :, om.neq - 1] if om.poisson else None
    if kind in ("e_r", "e_z"):
        assert om.poisson
        d = 0 if kind == "e_r" else 1
        return [[-Phi[:, a] * om.G[:, a, d] for a in range(3)] for _ in pts]
    if kind == "e_norm":
        assert om.poisson
        return [[Em] for _ in pts]
    if kind == "rate":
        k, P, _ = om.reactions[index]
        kv = k(Em)[0]
        out = []
        for phi, _ in pts:
            prod = np.ones(nc)
            for i in range(om.ns):
                if P[i]:
                    prod = prod * om._dens(Uc[:, :, i] @ phi)[0] ** P[i]
            out.append([kv * prod])
        return out
    assert kind in ("flux_r", "flux_z")
    d, s = (0 if kind == "flux_r" else 1), index
    if om.eq_type[s] == REACTION:
        return [[np.zeros(nc)] for _ in pts]
    Dv = om.D[s](Em)[0]
    dif = [-Dv * Uc[:, a, s] * om.G[:, a, d] for a in range(3)]             # -D grad u, corner by corner
    w = []
    if om.eq_type[s] == DRIFT_DIFFUSION_REACTION:
        if om.drift_w[s] is not None:
            w = [np.full(nc, float(om.drift_w[s][d]))]
        elif om.poisson:
            Zmu = om.Z[s] * om.mu[s](Em)[0]
            w = [-Zmu * Phi[:, a] * om.G[:, a, d] for a in range(3)]          # Z mu E, corner by corner
    out = []
    for phi, _ in pts:
        us = Uc[:, :, s] @ phi
        n = om._dens(us)[0]
        out.append([t * n for t in dif + w] if om.log else dif + [t * us for t in w])
    return out


def cell_magnitudes(om, U, kind):
    """Where the magnitudes of ``cell_integrands``' addends do not bound an implementation's rounding: E_NORM is one
    addend, |E|, formed from the two gradient components -- the addends of those bound it (|E| <= |dPhi/dr| + |dPhi/dz|
    <= sum_a |Phi_a| (|G_a0| + |G_a1|), and so does its rounding).  None for the other kinds."""
    if kind != "e_norm":
        return None
    Phi = np.asarray(U, dtype=np.float64)[om.mesh.cells][:, :, om.neq - 1]
    mags = [np.abs(Phi[:, a] * om.G[:, a, d]) for a in range(3) for d in range(2)]
    return [mags for _ in points(om)]


def load(om, integrands, magnitudes=None):
    """``Projected(b, abs, m)`` of the integrand given as ``cell_integrands`` gives it: per quadrature point a list of
    arrays [cell] whose sum is f(x_q).  ``magnitudes``: the same shape, what ``abs`` adds up instead of the addends'
    own magnitudes (``cell_magnitudes``)."""
    def corner_sets(per_point):
        return [[W * f * phi[a] for a in range(3)] for (phi, W), addends in zip(points(om), per_point) for f in addends]
    b, ab = _vertex_fsum(om, corner_sets(integrands))
    if magnitudes is not None:
        ab = _vertex_fsum(om, corner_sets(magnitudes))[1]
    return Projected(b, ab, lumped_mass(om))


def projected(om, U, kind, index=0):
    """``Projected(b, abs, m)`` of one projected kind at the state U[nv, neq]."""
    return load(om, cell_integrands(om, U, kind, index), cell_magnitudes(om, U, kind))


def pointwise(om, U, kind, index=0):
    U = np.asarray(U, dtype=np.float64)
    if kind == "state":
        return Pointwise(U[:, index].copy(), np.abs(U[:, index]))
    if kind == "density":
        n = om._dens(U[:, index])[0]
        return Pointwise(n, np.abs(n))
    assert kind == "charge"
    terms = [elementary_charge * om.Z[s] * om._dens(U[:, s].astype(np.longdouble))[0] for s in range(om.ns)]
    value = np.array(sum(terms), dtype=np.float64)
    return Pointwise(value, np.array(sum(np.abs(t) for t in terms), dtype=np.float64))


def reference(om, U, name):
    """``Projected`` or ``Pointwise`` of the field called ``name`` ("E_norm", "rate:0", ...)."""
    kind, index = parse(name)
    return projected(om, U, kind, index) if kind in PROJECTED else pointwise(om, U, kind, index)


def lumped(p):
    return p.b / p.m


def consistent(om, p):
    """X with M X = b, by a direct solve."""
    return spla.spsolve(mass_matrix(om).tocsc(), p.b)
