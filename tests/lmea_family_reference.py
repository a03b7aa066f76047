"""numpy restatement of the LMEA residual and Jacobian for the whole model family of ``fedm_gd_desc`` (helper module of
test_lmea_family_reference.py and test_gpu_lmea_family.py).

Written from the formulae documented in include/fedm_hip.h and the semantics of the reference's fedm/functions.py
(Flux :219-237, Source_term / Energy_Source_term :835-912, 'flux source' walls :514-522, semi_implicit_coefficients
:753-774), for any ``GdModel.to_c()``-shaped ``md``: 2 .. 5 species (the gas included), up to 16 reactions, planar or
axisymmetric, any tags.  The point functions (unknowns, dme, the semi-implicit mu, D and k, the addends of a flux) are
tests/balance_reference._Points -- one copy; this module adds the element residual around them, written once for
real and complex unknowns, and takes the Jacobian by the complex step (h = 1e-30), column by column of the element
matrix, as oracle/gd.py does.  ``Max(x, 0)`` and ``|x|`` follow the oracle's ``cabs``.

Every addend of the residual is filed under a class (`classes`): per dof row the sum of |addend| of the class over the
cells, points and facets that meet the row.  test_lmea_family_reference.py uses them to show that at the tests' states
no part of the formulae hides below the bounds the device is held to.

`PERTURBATIONS`: deliberate faults, each a change of the model copy, the field table or a switch the element residual
reads.  ``applies(md)`` says whether a model has the feature the fault needs.
"""
import copy
import types

import numpy as np
import scipy.sparse as sp

from balance_reference import (DIFFUSION_REACTION, DRIFT_DIFFUSION_REACTION, REACTION, _Points, geometry)
from oracle.gd import cabs

STEP = 1e-30


# ---- the model as plain lists (a copy a perturbation may change) --------------------------------------------------------
def plain_model(md):
    ns, nr, nt = int(md.n_species), int(md.n_reactions), int(md.n_tags)
    m = types.SimpleNamespace(
        n_species=ns, n_reactions=nr, n_tags=nt, axisymmetric=int(md.axisymmetric), N0=float(md.N0),
        charge_over_eps=float(md.charge_over_eps), eq_type=[int(md.eq_type[i]) for i in range(ns)],
        grad_diffusion=[int(md.grad_diffusion[i]) for i in range(ns)], is_ion=[int(md.is_ion[i]) for i in range(ns)],
        sign=[float(md.sign[i]) for i in range(ns)], vth=[float(md.vth[i]) for i in range(ns)],
        vth_e_coef=float(md.vth_e_coef), power=[[int(md.power[j][i]) for i in range(ns)] for j in range(nr)],
        net=[[int(md.net[j][i]) for i in range(ns)] for j in range(nr)],
        energy_loss=[float(md.energy_loss[j]) for j in range(nr)],
        ref=[[float(md.ref[t][i]) for i in range(ns)] for t in range(nt)], gamma=[float(md.gamma[t]) for t in range(nt)],
        we_secondary=float(md.we_secondary), energy_Ei=float(md.energy_Ei), mean_energy_form=int(md.mean_energy_form))
    # switches of the element residual that only a perturbation sets
    m.electron_square_derivative_as_one = False
    m.energy_drift_scale = 5.0 / 3.0
    return m


def sentinel_kind(loss):
    """1: the reaction loses (Ei - mean energy), 2: the mean energy itself, 0: the number"""
    return 1 if 7e77 < loss < 8e77 else 2 if 9e99 < loss < 1e100 else 0


def ions(m):
    return [s for s in range(1, m.n_species - 1) if m.is_ion[s]]


def heavy_with_flux(m):
    return [s for s in range(1, m.n_species - 1) if m.eq_type[s] != REACTION]


# ---- the deliberate faults ----------------------------------------------------------------------------------------------
def _drop_row(row_of):
    def change(m, fields):
        fields[row_of(m)] = 0.0
    return change


def _p_grad_diffusion(m, fields):
    s = [s for s in ions(m) if m.grad_diffusion[s] and m.eq_type[s] == DRIFT_DIFFUSION_REACTION][0]
    m.grad_diffusion[s] = 0


def _p_second_ion(m, fields):
    m.is_ion[ions(m)[1]] = 0


def _p_power4(m, fields):
    m.power = [[min(p, 3) if p == 4 else p for p in row] for row in m.power]


def _p_square(m, fields):
    m.electron_square_derivative_as_one = True


def _p_ref(m, fields):
    m.ref = [m.ref[(t - 1) % m.n_tags] for t in range(m.n_tags)]


def _p_we(m, fields):
    m.we_secondary = 1.0


def _p_axi(m, fields):
    m.axisymmetric = 0 if m.axisymmetric else 1


def _p_reaction_flux(m, fields):
    s = [s for s in range(1, m.n_species) if m.eq_type[s] == REACTION][0]
    m.eq_type[s] = DIFFUSION_REACTION


def _p_energy_drift(m, fields):
    m.energy_drift_scale = 1.0


def _p_Ei(m, fields):
    m.energy_Ei = 0.0


Perturbation = types.SimpleNamespace
PERTURBATIONS = {
    "an ion's grad_diffusion term dropped": Perturbation(
        change=_p_grad_diffusion, jacobian_only=False,
        applies=lambda m: any(m.grad_diffusion[s] and m.eq_type[s] == DRIFT_DIFFUSION_REACTION for s in ions(m))),
    "second ion left out of the emission sum": Perturbation(
        change=_p_second_ion, jacobian_only=False, applies=lambda m: len(ions(m)) > 1 and any(m.gamma)),
    "a power of 4 taken as 3": Perturbation(
        change=_p_power4, jacobian_only=False, applies=lambda m: any(4 in row for row in m.power)),
    "electron power 2 differentiated as 1": Perturbation(
        change=_p_square, jacobian_only=True, applies=lambda m: any(row[m.n_species - 1] == 2 for row in m.power)),
    "tag t's ref taken from tag t - 1": Perturbation(change=_p_ref, jacobian_only=False, applies=lambda m: m.n_tags > 1),
    "gamma not scaled by we_secondary in the energy row": Perturbation(
        change=_p_we, jacobian_only=False, applies=lambda m: bool(ions(m)) and any(m.gamma) and m.we_secondary != 1.0),
    "an ion's mu_d * dme dropped": Perturbation(
        change=_drop_row(lambda m: 2 * m.n_species + ions(m)[0]), jacobian_only=False,
        applies=lambda m: any(m.eq_type[s] == DRIFT_DIFFUSION_REACTION for s in ions(m)[:1])),
    "a heavy species' D_d * dme dropped": Perturbation(
        change=_drop_row(lambda m: 3 * m.n_species + heavy_with_flux(m)[0]), jacobian_only=False,
        applies=lambda m: bool(heavy_with_flux(m))),
    "the kd of one reaction dropped": Perturbation(
        change=_drop_row(lambda m: 4 * m.n_species + m.n_reactions), jacobian_only=False,
        applies=lambda m: m.n_reactions > 0),
    "planar and axisymmetric weights swapped": Perturbation(change=_p_axi, jacobian_only=False, applies=lambda m: True),
    "a reaction-type species given a flux": Perturbation(
        change=_p_reaction_flux, jacobian_only=False,
        applies=lambda m: any(m.eq_type[s] == REACTION for s in range(1, m.n_species))),
    "the 5/3 of the energy flux applied to D only": Perturbation(
        change=_p_energy_drift, jacobian_only=False, applies=lambda m: True),
    "sentinel kind-1 weight loses Ei": Perturbation(
        change=_p_Ei, jacobian_only=False,
        applies=lambda m: any(sentinel_kind(v) == 1 for v in m.energy_loss) and m.energy_Ei != 0.0),
}


# ---- the element residual -----------------------------------------------------------------------------------------------
class _Assembly:
    """Geometry, model copy and field table of one evaluation; `element_residual` for real or complex unknowns."""

    def __init__(self, m, coords, cells, tags, fields, Uo, Uo1, dt, dt_old, rules):
        self.m, self.cells = m, np.asarray(cells)
        self.tags = np.zeros((self.cells.shape[0], 3), dtype=np.int8) if tags is None else np.asarray(tags).reshape(-1, 3)
        self.fields = np.asarray(fields, dtype=np.float64)
        self.x, self.detJ, self.G = geometry(coords, self.cells)
        self.rn = self.x[:, :, 0] if m.axisymmetric else np.full(self.x.shape[:2], 0.5 / np.pi)
        self.Uoc, self.Uo1c = np.asarray(Uo, dtype=np.float64)[self.cells], np.asarray(Uo1, dtype=np.float64)[self.cells]
        self.dt, self.dt_old = float(dt), float(dt_old)
        (self.xq, self.wq), (self.tq, self.wt) = rules

    def _flux(self, pts, p, s):
        """the addends of the flux of species s by class: {class: (gx, gy)}"""
        m = self.m
        if m.eq_type[s] == REACTION:
            return {}
        drift = m.eq_type[s] == DRIFT_DIFFUSION_REACTION
        grad_d = bool(m.grad_diffusion[s]) if drift else True
        names = (["grad-D flux"] if grad_d else []) + ["diffusion flux"] + (["drift flux"] if drift else [])
        return dict(zip(names, pts.flux_addends(p, s)))

    def _energy_point(self, p):
        """the point as the energy flux sees it: u_0 in the electrons' place, 5/3 of their D and mu"""
        m = self.m
        ie = m.n_species - 1
        q = copy.copy(p)
        q.u, q.e, q.D, q.mu = list(p.u), list(p.e), list(p.D), list(p.mu)
        q.u[ie], q.e[ie] = p.u[0], p.e[0]
        D = p.D[ie]
        q.D[ie] = type(D)(D.v * (5.0 / 3.0), D.gx * (5.0 / 3.0), D.gy * (5.0 / 3.0))
        q.mu[ie] = p.mu[ie] * m.energy_drift_scale
        return q

    def element_residual(self, Uc, mags=None):
        """R[cells, 3, n_eq] for the cells' nodal unknowns Uc (real or complex); `mags`: a dict that receives, per
        class, the sums of |addend| in the same shape (real unknowns only)."""
        m = self.m
        ns, nr = m.n_species, m.n_reactions
        ie, iphi = ns - 1, ns
        G, cells = self.G, self.cells
        R = np.zeros(Uc.shape, dtype=Uc.dtype)
        tr = self.dt / self.dt_old
        trp1, tr2p1 = 1.0 + tr, 1.0 + 2.0 * tr
        two_pi = 2.0 * np.pi

        def add(name, cs, a, comp, val):
            R[cs, a, comp] += val
            if mags is not None:
                mags.setdefault(name, np.zeros(Uc.shape))[cs, a, comp] += np.abs(val)

        every = slice(None)
        pts = _Points(m, self.fields, None, cells, G, Uc=Uc)
        for xi, w in zip(self.xq, self.wq):
            phi = np.array([1.0 - xi[0] - xi[1], xi[0], xi[1]])
            W = w * self.detJ * two_pi * (self.rn @ phi)
            p = pts.at(phi)
            # reaction rates
            rate = []
            for j in range(nr):
                Rj = p.k[j]
                for i in range(ns):
                    pw = m.power[j][i]
                    if i == ie and pw == 2 and m.electron_square_derivative_as_one:
                        Rj = (Rj * np.real(p.e[i])) * p.e[i]       # the value of the square, half its derivative
                        continue
                    for _ in range(pw):
                        Rj = Rj * (m.N0 if i == 0 else p.e[i])
                rate.append(Rj)
            me_arg = p.u[0].v / p.u[ie].v if m.mean_energy_form == 1 else 0.0
            flux = {c: self._flux(pts, p, c) for c in range(1, ns)}
            flux[0] = self._flux(pts, self._energy_point(p), ie)
            joule = list(self._flux(pts, p, ie).values())
            for c in range(ns):
                T = p.e[c] * ((p.u[c].v * tr2p1 - trp1 ** 2 * (self.Uoc[:, :, c] @ phi) + tr ** 2 * (self.Uo1c[:, :, c] @ phi))
                              / trp1) / self.dt
                for a in range(3):
                    add("time term", every, a, c, W * T * phi[a])
                    for name, (gx, gy) in flux[c].items():
                        add(name, every, a, c, -W * (gx * G[:, a, 0] + gy * G[:, a, 1]))
                    for j in range(nr):
                        if c == 0:
                            kind = sentinel_kind(m.energy_loss[j])
                            if kind == 1:
                                add(f"sentinel share {j}", every, a, 0, W * ((m.energy_Ei - me_arg) * rate[j]) * phi[a])
                            elif kind == 2:
                                add(f"sentinel share {j}", every, a, 0, W * (me_arg * rate[j]) * phi[a])
                            elif m.energy_loss[j] != 0.0:
                                add(f"reaction {j} share", every, a, 0, W * (m.energy_loss[j] * rate[j]) * phi[a])
                        elif m.net[j][c]:
                            add(f"reaction {j} share", every, a, c, -W * (m.net[j][c] * rate[j]) * phi[a])
                    if c == 0:      # Joule heating: the source has -(Gamma_e . E)
                        for gx, gy in joule:
                            add("Joule heating", every, a, 0, W * (gx * p.Ex + gy * p.Ey) * phi[a])
            for a in range(3):
                add("Poisson gradient part", every, a, iphi, W * (p.u[iphi].gx * G[:, a, 0] + p.u[iphi].gy * G[:, a, 1]))
                for i in range(1, ns):
                    if m.sign[i] != 0.0:
                        add(f"charge part of species {i}", every, a, iphi, -W * (m.charge_over_eps * m.sign[i]) * p.e[i] * phi[a])

        # 'flux source' walls
        ends = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
        self.wall_signs = dict(ion=[], drift=[])
        for i in range(3):
            cs = np.nonzero(self.tags[:, i] > 0)[0]
            if cs.size == 0:
                continue
            j, kk = ends[i]
            t = self.tags[cs, i].astype(np.int64) - 1
            ref = np.array(m.ref)[t]                    # [facets, species]
            gam = np.array(m.gamma)[t]
            sub = _Points(m, self.fields, None, cells[cs], G[cs], Uc=Uc[cs])
            Gi = G[cs, i]
            gi = np.sqrt(Gi[:, 0] ** 2 + Gi[:, 1] ** 2)
            nx, ny = -Gi[:, 0] / gi, -Gi[:, 1] / gi
            e_ = self.x[cs, j] - self.x[cs, kk]
            L = np.sqrt(e_[:, 0] ** 2 + e_[:, 1] ** 2)
            for tq, w in zip(self.tq, self.wt):
                phi = np.zeros(3)
                phi[j], phi[kk] = 1.0 - tq, tq
                W = w * L * two_pi * (self.rn[cs] @ phi)
                p = sub.at(phi)
                En = p.Ex * nx + p.Ey * ny
                ion = 0.0
                for s in range(1, ns):
                    if not m.is_ion[s]:
                        continue
                    gn = sum(gx * nx + gy * ny for gx, gy in sub.flux_addends(p, s))
                    ion = ion + (gn + cabs(gn)) / 2.0                       # Max(., 0)
                    self.wall_signs["ion"].append(np.real(gn))
                vth_e = np.sqrt(m.vth_e_coef * p.me)
                for c in range(ns):
                    s = ie if c == 0 else c
                    if m.eq_type[s] == REACTION:
                        continue
                    fac = (1.0 - ref[:, s]) / (1.0 + ref[:, s])
                    vth = vth_e if s == ie else m.vth[s]
                    mu_scale, g = 1.0, gam
                    if c == 0:
                        vth, mu_scale, g = vth * 1.3333, 5.0 / 3.0, gam * m.we_secondary
                    parts = {"wall thermal part": fac * (0.5 * vth * p.e[c])}
                    if m.eq_type[s] != DIFFUSION_REACTION:
                        parts["wall drift part"] = fac * (cabs(m.sign[s] * mu_scale * p.mu[s] * En) * p.e[c])
                        self.wall_signs["drift"].append(np.real(m.sign[s] * p.mu[s] * En))
                        if s == ie and ions(m):
                            parts["wall emission part"] = -(2.0 * g / (1.0 + ref[:, s])) * ion
                    for name, val in parts.items():
                        for a in (j, kk):
                            add(name, cs, a, c, W * val * phi[a])
        return R


def _scatter(cells, n_eq, nv, Re):
    idx = (np.asarray(cells, dtype=np.int64)[:, :, None] * n_eq + np.arange(n_eq)[None, None, :]).ravel()
    return np.bincount(idx, weights=Re.ravel(), minlength=nv * n_eq)


def residual_jacobian(md, coords, cells, facet_tags, fields, U, Uo, Uo1, dt, dt_old, dirichlet_dofs, dirichlet_vals, rules,
                      perturbation=None, jacobian=True, classes=True):
    """F [n_dofs], J (scipy CSR, the rows of `dirichlet_dofs` identity rows) and the classes' magnitudes per row.

    ``fields[n_fields, nv]`` in the order of ``FEDM_GD_N_FIELDS``; ``facet_tags[nc, 3]``: facet i lies opposite vertex i;
    ``rules = ((points[nq, 2], weights[nq]), (t[nf], weights[nf]))`` on the reference triangle and the unit interval;
    ``perturbation``: a key of `PERTURBATIONS`.  Returns a namespace with F, J (None without ``jacobian``), ``classes``
    ({class: [n_dofs]}, the constrained rows zero), ``pattern`` (boolean CSR: the positions of J whose row and column fields
    are coupled in some element matrix, for every pair of vertices that share a cell, and the constrained rows' diagonal) and ``wall_signs`` (the values of Gamma_i . n and of
    sign mu E_n met at the wall points)."""
    m = plain_model(md)
    fields = np.array(fields, dtype=np.float64)
    if perturbation is not None:
        PERTURBATIONS[perturbation].change(m, fields)
    cells = np.asarray(cells)
    U = np.asarray(U, dtype=np.float64)
    nv, neq = U.shape
    assert neq == m.n_species + 1
    asm = _Assembly(m, coords, cells, facet_tags, fields, Uo, Uo1, dt, dt_old, rules)
    Uc = U[cells]
    mags = {} if classes else None
    Re = asm.element_residual(Uc, mags)
    ddofs = np.asarray(dirichlet_dofs, dtype=np.int64)
    F = _scatter(cells, neq, nv, Re)
    F[ddofs] = U.ravel()[ddofs] - np.asarray(dirichlet_vals, dtype=np.float64)
    out = types.SimpleNamespace(F=F, J=None, classes=None, pattern=None, wall_signs=asm.wall_signs, model=m)
    if classes:
        out.classes = {}
        for name, M in mags.items():
            out.classes[name] = _scatter(cells, neq, nv, M)
            out.classes[name][ddofs] = 0.0
    if not jacobian:
        return out
    nc = cells.shape[0]
    Ke = np.empty((nc, 3, neq, 3, neq))
    for b in range(3):
        for s in range(neq):
            Up = Uc.astype(np.complex128)
            Up[:, b, s] += 1j * STEP
            Ke[:, :, :, b, s] = np.imag(asm.element_residual(Up)) / STEP
    c = cells.astype(np.int64)
    shape = (nc, 3, neq, 3, neq)
    rows = np.broadcast_to(c[:, :, None, None, None] * neq + np.arange(neq)[None, None, :, None, None], shape).ravel()
    cols = np.broadcast_to(c[:, None, None, :, None] * neq + np.arange(neq)[None, None, None, None, :], shape).ravel()
    N = nv * neq
    keep = np.ones(N)
    keep[ddofs] = 0.0
    eye = sp.coo_matrix((np.ones(ddofs.size), (ddofs, ddofs)), shape=(N, N))
    out.J = (sp.diags(keep) @ sp.coo_matrix((Ke.ravel(), (rows, cols)), shape=(N, N)).tocsr() + eye).tocsr()
    # the pattern is structural: (row field, column field) pairs that are coupled in some element matrix, at every pair of
    # vertices that share a cell -- an entry that is zero because two edges of a cell are perpendicular is still in it
    coupled = (Ke != 0.0).any(axis=(0, 1, 3))
    hit = np.broadcast_to(coupled[None, None, :, None, :], shape).ravel()
    pat = sp.coo_matrix((np.ones(int(hit.sum())), (rows[hit], cols[hit])), shape=(N, N)).tocsr()
    out.pattern = ((sp.diags(keep) @ pat + eye).tocsr() != 0).tocsr()
    out.coupled = coupled
    return out
