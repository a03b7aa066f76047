"""numpy restatement of the electrode currents (helper module of the currents tests).

Written from the formulae of include/fedm_hip.h (fedm_currents), independently of csrc/currents.hip.  The point functions
are not restated here: the LFA family's geometry, cell fields, densities and coefficients are ``oracle.forms.LFAModel``'s
through tests/diagnostics_reference.py (``points``), the LMEA family's unknowns, dme, semi-implicit coefficients and flux
addends are tests/balance_reference.py's (``geometry``, ``_Points``).

    W_q            = w_q |det J| 2 pi w(x_q)                         w = r (axisymmetric) or 1/(2 pi)
    conduction[g]  = sum_s Z_s sum W Gamma_s . (-grad psi_g)         LMEA: s >= 1, Z_s = sign_s
    D_t Phi        = ((1 + 2w) Phi - (1 + w)^2 Phi_old + w^2 Phi_old1) / ((1 + w) dt),   w = dt / dt_old,   nodal
    displacement[g]= sum W grad(D_t Phi) . grad psi_g
    coupling[g]    = sum W grad Phi . grad psi_g
    induced_charge[g] = sum_s Z_s sum W n_s psi_g
    capacitance[g][h] = sum W grad psi_g . grad psi_h

Every sum comes back as ``Sum(value, abs)``: ``math.fsum`` of its terms and the sum of their magnitudes.  A term is one
addend as an implementation forms it in floating point before it adds: for the conduction each flux addend (diffusion,
drift) times each component of grad psi at each quadrature point; for the gradient products each vertex's nodal value
times its basis gradient, per component (and for the displacement per BDF2 addend); for the charge each species at each
quadrature point and vertex.

``faults``: names of deliberate mistakes (FAULTS), for the tests that show the bound sees them ("a reaction species'
flux kept" is the LFA family's: no LMEA model of the tests has a charged 'reaction' species; "sign_s left out" is the
LMEA family's).
tests/test_currents_reference.py pins this module on closed forms; tests/test_gpu_currents.py holds the device to it.
"""
import math
from collections import namedtuple

import numpy as np

import balance_reference as bref
import diagnostics_reference as dref

Sum = namedtuple("Sum", "value abs")
FAULTS = ("equal-step BDF2 weights", "u_old1 taken for u_old", "+grad psi", "a reaction species' flux kept",
          "sign_s left out", "planar weight taken as 1")
OUTPUTS = ("conduction", "displacement", "coupling", "induced_charge")


def _sum(arrays):
    flat = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]) if arrays else np.zeros(0)
    return Sum(math.fsum(flat.tolist()), math.fsum(np.abs(flat).tolist()))


def bdf2_weights(dt, dt_old, equal_step=False):
    """(c_new, c_old, c_old1) / dt of the variable-step BDF2 quotient."""
    w = 1.0 if equal_step else dt / dt_old
    return np.array([(1.0 + 2.0 * w) / (1.0 + w), -(1.0 + w), w * w / (1.0 + w)]) / dt


def _assemble(cells, G, Wtot, flux_addends, charge_addends, Phis, dt, dt_old, psis, faults):
    """``flux_addends``: [(jx[nc], jy[nc])], each Z_s W Gamma_s-addend at one quadrature point; ``charge_addends``:
    [(coef[nc], phi[3])], each Z_s W n_s at one point with the basis there; ``Phis``: the potential's nodal values of
    u_new, u_old, u_old1."""
    psis = np.atleast_2d(np.asarray(psis, dtype=np.float64))
    Phi, Phio, Phio1 = (np.asarray(p, dtype=np.float64) for p in Phis)
    if "u_old1 taken for u_old" in faults:
        Phio = Phio1
    cw = bdf2_weights(dt, dt_old, "equal-step BDF2 weights" in faults)
    sgn = 1.0 if "+grad psi" in faults else -1.0
    gpsi = [np.einsum("ca,cad->cd", p[cells], G) for p in psis]
    out = {k: [] for k in OUTPUTS}
    for g, p in enumerate(psis):
        gp = gpsi[g]
        out["conduction"].append(_sum([sgn * j[d] * gp[:, d] for j in flux_addends for d in range(2)]))
        out["displacement"].append(_sum([Wtot * c * P[cells[:, a]] * G[:, a, d] * gp[:, d]
                                         for c, P in zip(cw, (Phi, Phio, Phio1)) for a in range(3) for d in range(2)]))
        out["coupling"].append(_sum([Wtot * Phi[cells[:, a]] * G[:, a, d] * gp[:, d] for a in range(3) for d in range(2)]))
        out["induced_charge"].append(_sum([coef * phi[a] * p[cells[:, a]] for coef, phi in charge_addends for a in range(3)]))
    n = len(psis)
    cap = [[None] * n for _ in range(n)]
    for g in range(n):
        for h in range(g, n):
            cap[g][h] = cap[h][g] = _sum([Wtot * psis[g][cells[:, a]] * G[:, a, d] * psis[h][cells[:, b]] * G[:, b, d]
                                          for a in range(3) for b in range(3) for d in range(2)])
    out["capacitance"] = cap
    return out


def lfa_reference(om, U, Uo, Uo1, dt, dt_old, psis, faults=()):
    """dict(conduction, displacement, coupling, induced_charge: [Sum]; capacitance: [[Sum]]) of an LFA model with a
    Poisson equation (``om``: the oracle's) at the states U, Uo, Uo1 [nv, neq]."""
    from oracle.forms import DRIFT_DIFFUSION_REACTION, REACTION
    assert om.poisson
    U = np.asarray(U, dtype=np.float64)
    ns, nc, cells = om.ns, om.mesh.nc, om.mesh.cells
    Uc, E, Em = om.cell_fields(U)
    scale = 2.0 * np.pi if ("planar weight taken as 1" in faults and not om.axisymmetric) else 1.0
    pts = [(phi, W * scale) for phi, W, _ in dref.points(om)]
    Wtot = sum(W for _, W in pts)
    flux, charge = [], []
    for s in range(ns):
        dens = [om._dens(Uc[:, :, s] @ phi)[0] for phi, _ in pts]
        for (phi, W), n in zip(pts, dens):
            charge.append((om.Z[s] * W * n, phi))
        if om.eq_type[s] == REACTION and "a reaction species' flux kept" not in faults:
            continue
        gradu = np.einsum("ca,cad->cd", Uc[:, :, s], om.G)
        dif = -om.D[s](Em)[0][:, None] * gradu
        drift = None
        if om.eq_type[s] in (DRIFT_DIFFUSION_REACTION, REACTION):
            if om.drift_w[s] is not None:
                drift = np.broadcast_to(np.asarray(om.drift_w[s], dtype=np.float64)[None, :], (nc, 2))
            else:
                drift = (om.Z[s] * om.mu[s](Em)[0])[:, None] * E
        for (phi, W), n in zip(pts, dens):
            f = om.Z[s] * W * (n if om.log else 1.0)
            flux.append((f * dif[:, 0], f * dif[:, 1]))
            if drift is not None:
                f = om.Z[s] * W * n
                flux.append((f * drift[:, 0], f * drift[:, 1]))
    np_ = om.ns
    return _assemble(cells, om.G, Wtot, flux, charge, (U[:, np_], np.asarray(Uo)[:, np_], np.asarray(Uo1)[:, np_]), dt,
                     dt_old, psis, faults)


def lmea_reference(md, coords, cells, fields, U, Uo, Uo1, dt, dt_old, qp, psis, planar=None, faults=()):
    """The same of an LMEA model (``md``: ``fedm_gd_desc``-shaped) with the field table ``fields[n_fields, nv]``;
    ``qp = (points[nq, 2], weights[nq])`` on the reference triangle."""
    cells = np.asarray(cells)
    U = np.asarray(U, dtype=np.float64)
    ns = int(md.n_species)
    axi = bool(md.axisymmetric) if planar is None else not planar
    x, detJ, G = bref.geometry(coords, cells)
    rn = x[:, :, 0] if axi else np.full(x.shape[:2], 1.0 if "planar weight taken as 1" in faults else 0.5 / np.pi)
    pts = bref._Points(md, fields, U, cells, G)
    sign = [1.0 if "sign_s left out" in faults else float(md.sign[i]) for i in range(ns)]
    flux, charge, Wtot = [], [], 0.0
    for xi, w in zip(*qp):
        phi = np.array([1.0 - xi[0] - xi[1], xi[0], xi[1]])
        W = w * detJ * (2.0 * np.pi) * (rn @ phi)
        Wtot = Wtot + W
        p = pts.at(phi)
        for s in range(1, ns):
            charge.append((sign[s] * W * p.e[s], phi))
            for gx, gy in pts.flux_addends(p, s):
                flux.append((sign[s] * W * gx, sign[s] * W * gy))
    return _assemble(cells, G, Wtot, flux, charge, (U[:, ns], np.asarray(Uo)[:, ns], np.asarray(Uo1)[:, ns]), dt, dt_old,
                     psis, faults)


def combine(sums, weights):
    """A signed combination of Sums: Sum(fsum of w value, sum of |w| abs)."""
    return Sum(math.fsum(w * s.value for w, s in zip(weights, sums)), math.fsum(abs(w) * s.abs for w, s in zip(weights, sums)))


def test_potentials(coords, box, n_psi, r0=0.0):
    """``n_psi`` potentials z/box + 0.2 ((r - r0)/box)^2, scaled and shifted per slot so that no two are proportional."""
    r, z = (np.asarray(coords)[:, 0] - r0) / box, np.asarray(coords)[:, 1] / box
    return np.stack([(1.0 + 0.35 * k) * z + 0.2 * (1.0 - 0.11 * k) * r ** 2 + 0.05 * k * k * r * z + 0.03 * k
                     for k in range(n_psi)])


test_potentials.__test__ = False
