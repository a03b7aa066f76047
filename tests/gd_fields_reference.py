"""numpy restatement of the LMEA field output (helper module of the gd-fields tests).

Written from the table of include/fedm_hip.h (fedm_gd_fields), independently of csrc/gd_fields.hip, for any
``fedm_gd_desc``-shaped model ``md``, a mesh, the nodal field table ``fields[n_fields, nv]`` and a state ``U[nv, ns + 1]``.
The residual's point functions are tests/balance_reference.py's ``_Points`` (unknowns, dme, semi-implicit mu, D, k, the
fluxes' addends) with its ``geometry`` and ``loss_factor``: there is no second copy of them here.

    pointwise   STATE e  u_e(v)      DENSITY c  exp(u_c(v))     CHARGE  e sum_(s>=1) sign_s exp(u_s(v))
                MEAN_ENERGY  exp(u_0(v) - u_e(v))               TABLE f  fields[f][v]
    projected   E_R, E_Z, E_NORM, REDUCED_FIELD = 1e21 |grad Phi| / N0            (the potential alone)
                RATE j, SOURCE s, COLLISION_LOSS, JOULE, FLUX_R/Z c, CURRENT_R/Z    (the residual's point functions)

Projection in the plain measure: b_v = sum_(c with v) sum_q w_q |det J_c| f(x_q) phi_v(x_q), m_v = sum |det J_c| / 6.

A projected kind comes back as ``Projected(b, abs, m)``: ``b_v`` the ``math.fsum`` of its terms, ``abs`` the sum of their
magnitudes.  A term is ``w_q |det J| t phi_v`` for an addend ``t`` as balance_reference.py defines addends: a flux's
diffusion and drift addends separately (through JOULE and the currents, there per species), each reaction's share of a
source or of the loss, one addend for a rate; a gradient component of the potential is one addend, as it is in
balance_reference.py (the gradient part of a Poisson row, the drift addend mu E n of a flux: E is a cell's own number
there, not three corner products), and so are |E| and the reduced field.  (On the models of tests/lmea_models.py the
potential carries nodal noise of 0.3 E h on a drop of E L, so a cell's radial component is a thirtieth to an eightieth of
the corner products it is formed from: their rounding, 3 eps |Phi| / h, stays tens of times below 1e-12 |E_r|.)  Pointwise kinds
come back as ``Pointwise(value, abs)``.

``fault``: one of FAULTS, a deliberate mistake of the restatement (tests/test_gd_fields_reference.py shows that each
misses the device's bounds by far).
"""
import copy
import math
from collections import namedtuple

import numpy as np

import balance_reference as bref

Projected = namedtuple("Projected", "b abs m")
Pointwise = namedtuple("Pointwise", "value abs")
ELEMENTARY_CHARGE = 1.6021766208e-19
POINTWISE = ("state", "density", "charge", "mean_energy", "table")
POTENTIAL_ONLY = ("e_r", "e_z", "e_norm", "reduced_field")
OF_THE_STEP = ("rate", "source", "collision_loss", "joule", "flux_r", "flux_z", "current_r", "current_z")
PROJECTED = POTENTIAL_ONLY + OF_THE_STEP
FAULTS = ("the 5/3 left off the energy flux", "net taken for power", "a sentinel loss taken literally",
          "mu_d * dme dropped", "the gas included in the charge")


def parse(name):
    """(kind, index) of a name such as "E_norm", "rate:0", "flux_z:1"."""
    head, _, tail = name.partition(":")
    kind = head.lower()
    assert kind in POINTWISE + PROJECTED, name
    return kind, int(tail) if tail else 0


class Restatement:
    def __init__(self, md, coords, cells, fields, qp, fault=None):
        assert fault is None or fault in FAULTS
        self.md, self.fields, self.qp, self.fault = md, np.asarray(fields, dtype=np.float64), qp, fault
        self.coords, self.cells = np.asarray(coords, dtype=np.float64), np.asarray(cells)
        self.nv, self.nc = self.coords.shape[0], self.cells.shape[0]
        self.ns, self.nr = int(md.n_species), int(md.n_reactions)
        self.x, self.detJ, self.G = bref.geometry(self.coords, self.cells)
        self._where = [[] for _ in range(self.nv)]            # vertex -> flat (cell, corner) places, ascending
        for k, v in enumerate(self.cells.ravel().tolist()):
            self._where[v].append(k)
        self.m = np.array([math.fsum((self.detJ[k // 3] / 6.0) for k in w) for w in self._where])

    # ---- projection ---------------------------------------------------------------------------------------------------
    def points(self):
        """[(phi[3], W[cell])]: the basis at the model's quadrature points and w_q |det J| there"""
        return [(np.array([1.0 - xi[0] - xi[1], xi[0], xi[1]]), w * self.detJ) for xi, w in zip(*self.qp)]

    def _load(self, integrands, magnitudes=None):
        """``integrands``: per quadrature point a list of arrays [cell] whose sum is f(x_q)"""
        def terms(per_point):
            out = [(W * f)[:, None] * phi[None, :] for (phi, W), addends in zip(self.points(), per_point) for f in addends]
            return np.stack([t.ravel() for t in out]) if out else np.zeros((0, 3 * self.nc))
        T = terms(integrands)
        A = np.abs(T) if magnitudes is None else np.abs(terms(magnitudes))
        b = np.array([math.fsum(T[:, w].ravel().tolist()) for w in self._where])
        ab = np.array([math.fsum(A[:, w].ravel().tolist()) for w in self._where])
        return Projected(b, ab, self.m)

    def mass_matrix(self):
        import scipy.sparse as sp
        c = self.cells.astype(np.int64)
        M = sp.csr_matrix((self.nv, self.nv))
        for a in range(3):
            for b in range(3):
                M = M + sp.coo_matrix((self.detJ * (2.0 if a == b else 1.0) / 24.0, (c[:, a], c[:, b])), shape=M.shape).tocsr()
        return M.tocsr()

    @staticmethod
    def lumped(p):
        return p.b / p.m

    def consistent(self, p):
        import scipy.sparse.linalg as spla
        return spla.spsolve(self.mass_matrix().tocsc(), p.b)

    # ---- integrands ---------------------------------------------------------------------------------------------------
    def _point(self, pts, phi):
        p = pts.at(phi)
        if self.fault == "mu_d * dme dropped":
            p.mu = [pts.nodal(i, phi).v for i in range(self.ns)]
        return p

    def _energy_flux_addends(self, pts, p):
        """the energy row's flux: the electrons' flux formula on u_0 with 5/3 D_e and 5/3 mu_e"""
        ie = self.ns - 1
        s = 1.0 if self.fault == "the 5/3 left off the energy flux" else 5.0 / 3.0
        q = copy.copy(p)
        q.u, q.e, q.D, q.mu = list(p.u), list(p.e), list(p.D), list(p.mu)
        q.u[ie], q.e[ie] = p.u[0], p.e[0]
        q.D[ie] = bref._SG(p.D[ie].v * s, p.D[ie].gx * s, p.D[ie].gy * s)
        q.mu[ie] = p.mu[ie] * s
        return pts.flux_addends(q, ie)

    def _rate(self, p, j):
        md = self.md
        R = p.k[j]
        for i in range(self.ns):
            for _ in range(int(md.power[j][i])):
                R = R * (float(md.N0) if i == 0 else p.e[i])
        return R

    def cell_integrands(self, U, kind, index):
        """(integrands, magnitudes or None)"""
        md, ns, nr, ie = self.md, self.ns, self.nr, self.ns - 1
        U = np.asarray(U, dtype=np.float64)
        pts = bref._Points(md, self.fields, U, self.cells, self.G)
        npts = len(self.qp[1])
        if kind in POTENTIAL_ONLY:
            Phi = U[self.cells][:, :, ns]
            gx, gy = np.einsum("ca,ca->c", Phi, self.G[:, :, 0]), np.einsum("ca,ca->c", Phi, self.G[:, :, 1])
            Em = np.sqrt(gx * gx + gy * gy)
            f = {"e_r": -gx, "e_z": -gy, "e_norm": Em, "reduced_field": 1e21 * Em / float(md.N0)}[kind]
            return [[f] for _ in range(npts)], None
        out = []
        zero = np.zeros(self.nc)
        for phi, _ in self.points():
            p = self._point(pts, phi)
            if kind == "rate":
                out.append([self._rate(p, index)])
            elif kind == "source":
                table = md.power if self.fault == "net taken for power" else md.net
                out.append([float(table[j][index]) * self._rate(p, j) for j in range(nr) if int(table[j][index])] or [zero])
            elif kind == "collision_loss":
                me_arg = p.u[0].v / p.u[ie].v if int(md.mean_energy_form) == 1 else 0.0
                lf = (lambda j: float(md.energy_loss[j])) if self.fault == "a sentinel loss taken literally" else \
                    (lambda j: bref.loss_factor(md, j, me_arg))
                out.append([lf(j) * self._rate(p, j) for j in range(nr)])
            elif kind == "joule":
                out.append([t for gx, gy in pts.flux_addends(p, ie) for t in (-gx * p.Ex, -gy * p.Ey)])
            elif kind in ("flux_r", "flux_z"):
                d = 0 if kind == "flux_r" else 1
                adds = self._energy_flux_addends(pts, p) if index == 0 else pts.flux_addends(p, index)
                out.append([g[d] for g in adds] or [zero])
            else:
                assert kind in ("current_r", "current_z")
                d = 0 if kind == "current_r" else 1
                out.append([ELEMENTARY_CHARGE * float(md.sign[s]) * g[d] for s in range(1, ns) for g in pts.flux_addends(p, s)]
                           or [zero])
        return out, None

    def projected(self, U, kind, index=0):
        return self._load(*self.cell_integrands(U, kind, index))

    def pointwise(self, U, kind, index=0):
        U = np.asarray(U, dtype=np.float64)
        ns = self.ns
        if kind == "state":
            return Pointwise(U[:, index].copy(), np.abs(U[:, index]))
        if kind == "table":
            return Pointwise(self.fields[index].copy(), np.abs(self.fields[index]))
        if kind == "density":
            n = np.exp(U[:, index])
            return Pointwise(n, n)
        if kind == "mean_energy":
            return Pointwise(np.exp(U[:, 0] - U[:, ns - 1]), np.abs(U[:, 0] - U[:, ns - 1]))     # (abs: the exponent's size)
        assert kind == "charge"
        first = 0 if self.fault == "the gas included in the charge" else 1
        terms = [ELEMENTARY_CHARGE * float(self.md.sign[s]) * np.exp(U[:, s].astype(np.longdouble)) for s in range(first, ns)]
        return Pointwise(np.array(sum(terms), dtype=np.float64), np.array(sum(np.abs(t) for t in terms), dtype=np.float64))

    def reference(self, U, name):
        kind, index = parse(name)
        return self.projected(U, kind, index) if kind in PROJECTED else self.pointwise(U, kind, index)


def of_case(c, fault=None, md=None):
    """The restatement of a tests/lmea_models.case"""
    return Restatement(c.md if md is None else md, c.mesh.coords, c.mesh.cells, c.fields, c.rules[0], fault=fault)
