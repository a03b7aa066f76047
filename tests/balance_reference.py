"""numpy restatement of the LMEA balance (helper module of the balance tests).

Written from the formulae of include/fedm_hip.h (fedm_gd_balance), independently of csrc/gd_balance.hip, for any
``fedm_gd_desc``-shaped model ``md`` (``GdModel.to_c()`` or an object with its attributes), a mesh, the nodal field table
``fields[n_fields, nv]`` in the order of ``FEDM_GD_N_FIELDS`` and the three states.  ``planar``: None takes the model's
``axisymmetric``; True weighs with 1/(2 pi) in place of r.

Every sum comes back as ``Sum(value, abs, plain)``: ``math.fsum`` of its terms, the sum of their magnitudes, and the
terms added one after the other in float64 (cell-major order) -- ``plain - value`` is what the order of a float64
summation alone can move.  A term is one addend of the formula at one quadrature point, as an implementation forms it in
floating point before it adds: for ``rate_of_change`` the three BDF2 addends separately; for a flux its diffusion and
drift addends separately (through ``joule``, ``induced_current``, ``ion_flux`` and the emission part of ``wall``); for
``collision_loss`` each reaction's share; for a Poisson row the gradient part and each species' charge part.  Every
maximum comes back as ``Max(value, index, unique, centroid)`` like tests/diagnostics_reference.py.

tests/test_balance_reference.py pins this module on the oracle's element residual and on closed forms;
tests/test_gpu_balance.py holds the device to it.
"""
import math
from collections import namedtuple

import numpy as np

Sum = namedtuple("Sum", "value abs plain")
Max = namedtuple("Max", "value index unique centroid")
REACTION, DIFFUSION_REACTION, DRIFT_DIFFUSION_REACTION = 0, 1, 2


def _sum(terms, abs_terms=None):
    flat = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in terms]) if terms else np.zeros(0)
    mags = flat if abs_terms is None else (np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in abs_terms])
                                           if abs_terms else np.zeros(0))
    plain = float(np.cumsum(flat)[-1]) if flat.size else 0.0
    return Sum(math.fsum(flat.tolist()), math.fsum(np.abs(mags).tolist()), plain)


def _max(values, centroids=None):
    if values.size == 0:
        return Max(0.0, -1, True, None if centroids is None else (0.0, 0.0))
    top = values.max()
    at = np.nonzero(values == top)[0]
    c = None if centroids is None else (float(centroids[at[0], 0]), float(centroids[at[0], 1]))
    return Max(float(top), int(at[0]), at.size == 1, c)


class _SG:
    """value and spatial gradient of a P1 field at a point of every cell"""

    def __init__(self, v, gx, gy):
        self.v, self.gx, self.gy = v, gx, gy


def geometry(coords, cells):
    x = np.asarray(coords, dtype=np.float64)[cells]
    d1, d2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    det = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
    G = np.empty_like(x)
    G[:, 0, 0] = (x[:, 1, 1] - x[:, 2, 1]) / det
    G[:, 0, 1] = (x[:, 2, 0] - x[:, 1, 0]) / det
    G[:, 1, 0] = (x[:, 2, 1] - x[:, 0, 1]) / det
    G[:, 1, 1] = (x[:, 0, 0] - x[:, 2, 0]) / det
    G[:, 2, 0] = (x[:, 0, 1] - x[:, 1, 1]) / det
    G[:, 2, 1] = (x[:, 1, 0] - x[:, 0, 0]) / det
    return x, np.abs(det), G


class _Points:
    """The residual's point functions on a subset of the cells: unknowns, dme, semi-implicit mu, D, k, the fluxes.
    ``Uc``: the cells' own nodal unknowns [cells, 3, n_eq] in place of ``U[cells]``; they may be complex (the
    complex-step Jacobian of tests/lmea_family_reference.py), and everything at a point then is."""

    def __init__(self, md, fields, U, cells, G, Uc=None):
        self.md, self.fields, self.cells, self.G = md, np.asarray(fields, dtype=np.float64), cells, G
        self.Uc = np.asarray(U, dtype=np.float64)[cells] if Uc is None else Uc
        self.ns, self.nr = int(md.n_species), int(md.n_reactions)

    def sg(self, A, phi):
        return _SG(A @ phi, np.einsum("ca,ca->c", A, self.G[:, :, 0]), np.einsum("ca,ca->c", A, self.G[:, :, 1]))

    def nodal(self, row, phi):
        return self.sg(self.fields[row][self.cells], phi)

    def at(self, phi):
        ns, nr = self.ns, self.nr
        F_MEO = 4 * ns + 2 * nr
        p = type("P", (), {})()
        p.phi = phi
        p.u = [self.sg(self.Uc[:, :, i], phi) for i in range(ns + 1)]
        p.e = [np.exp(p.u[i].v) for i in range(ns)]
        p.Ex, p.Ey = -p.u[ns].gx, -p.u[ns].gy
        meo, ueo = self.nodal(F_MEO, phi), self.nodal(F_MEO + 2, phi)
        p.me = self.nodal(F_MEO + 1, phi).v
        e0, ee, eo = p.e[0], p.e[ns - 1], np.exp(ueo.v)
        num = _SG(e0 - ee * meo.v, e0 * p.u[0].gx - (ee * p.u[ns - 1].gx * meo.v + ee * meo.gx),
                  e0 * p.u[0].gy - (ee * p.u[ns - 1].gy * meo.v + ee * meo.gy))
        inv = 1.0 / eo
        p.dme = _SG(num.v * inv, (num.gx - num.v * inv * (eo * ueo.gx)) * inv, (num.gy - num.v * inv * (eo * ueo.gy)) * inv)
        p.mu, p.D = [], []
        for i in range(ns):
            p.mu.append(self.nodal(i, phi).v + self.nodal(2 * ns + i, phi).v * p.dme.v)
            Da, Db = self.nodal(ns + i, phi), self.nodal(3 * ns + i, phi)
            p.D.append(_SG(Da.v + Db.v * p.dme.v, Da.gx + (Db.gx * p.dme.v + Db.v * p.dme.gx),
                           Da.gy + (Db.gy * p.dme.v + Db.v * p.dme.gy)))
        p.k = [self.nodal(4 * ns + j, phi).v + self.nodal(4 * ns + nr + j, phi).v * p.dme.v for j in range(nr)]
        return p

    def flux_addends(self, p, s):
        """[(gx, gy)] addends of the flux of species s: the diffusion addends, then the drift addend."""
        md = self.md
        et = int(md.eq_type[s])
        if et == REACTION:
            return []
        u, e, D = p.u[s], p.e[s], p.D[s]
        drift = et == DRIFT_DIFFUSION_REACTION
        grad_diffusion = bool(md.grad_diffusion[s]) if drift else True
        out = []
        if grad_diffusion:
            out.append((-D.gx * e, -D.gy * e))
        out.append((-D.v * (e * u.gx), -D.v * (e * u.gy)))
        if drift:
            sg = float(md.sign[s])
            out.append((sg * (p.mu[s] * p.Ex * e), sg * (p.mu[s] * p.Ey * e)))
        return out


def loss_factor(md, j, me_arg):
    lj = float(md.energy_loss[j])
    if 7e77 < lj < 8e77:
        return float(md.energy_Ei) - me_arg
    if 9e99 < lj < 1e100:
        return me_arg
    return lj


def reference(md, coords, cells, tags, fields, U, Uo, Uo1, dt, dt_old, qp, fqp, psi=None, group=None, n_groups=0,
              planar=None):
    """dict of every quantity of fedm_gd_balance.  ``qp = (points[nq, 2], weights[nq])`` on the reference triangle,
    ``fqp = (t[nf], weights[nf])`` on the unit interval; ``tags[nc, 3]``: facet i lies opposite vertex i."""
    cells = np.asarray(cells)
    U, Uo, Uo1 = (np.asarray(a, dtype=np.float64) for a in (U, Uo, Uo1))
    ns, nr, nt = int(md.n_species), int(md.n_reactions), int(md.n_tags)
    ie = ns - 1
    axi = bool(md.axisymmetric) if planar is None else not planar
    x, detJ, G = geometry(coords, cells)
    rn = x[:, :, 0] if axi else np.full(x.shape[:2], 0.5 / np.pi)
    two_pi = 2.0 * np.pi
    pts = _Points(md, fields, U, cells, G)
    Uoc, Uo1c = Uo[cells], Uo1[cells]
    tr = dt / dt_old
    trp1, tr2p1 = 1.0 + tr, 1.0 + 2.0 * tr
    sign = [float(md.sign[i]) for i in range(ns)]
    coe = float(md.charge_over_eps)

    content = [[] for _ in range(ns)]
    rate = [[] for _ in range(ns)]
    reac = [[] for _ in range(nr)]
    loss, joule, cur = [], [], []
    mp = None
    if psi is not None:
        pc = np.asarray(psi, dtype=np.float64)[cells]
        mp = (-np.einsum("ca,ca->c", pc, G[:, :, 0]), -np.einsum("ca,ca->c", pc, G[:, :, 1]))
    grp = None if not n_groups else np.asarray(group)[cells]
    gterms = [[] for _ in range(n_groups)]
    gP = (np.einsum("ca,ca->c", U[cells][:, :, ns], G[:, :, 0]), np.einsum("ca,ca->c", U[cells][:, :, ns], G[:, :, 1]))
    for xi, w in zip(*qp):
        phi = np.array([1.0 - xi[0] - xi[1], xi[0], xi[1]])
        W = w * detJ * two_pi * (rn @ phi)
        p = pts.at(phi)
        for c in range(ns):
            content[c].append(W * p.e[c])
            f = W * p.e[c] / (trp1 * dt)
            rate[c] += [f * tr2p1 * p.u[c].v, -f * trp1 ** 2 * (Uoc[:, :, c] @ phi), f * tr ** 2 * (Uo1c[:, :, c] @ phi)]
        me_arg = p.u[0].v / p.u[ie].v if int(md.mean_energy_form) == 1 else 0.0
        for j in range(nr):
            R = p.k[j]
            for i in range(ns):
                for _ in range(int(md.power[j][i])):
                    R = R * (float(md.N0) if i == 0 else p.e[i])
            reac[j].append(W * R)
            loss.append(W * loss_factor(md, j, me_arg) * R)
        for gx, gy in pts.flux_addends(p, ie):
            joule += [-W * gx * p.Ex, -W * gy * p.Ey]
        if mp is not None:
            for s in range(1, ns):
                for gx, gy in pts.flux_addends(p, s):
                    cur += [sign[s] * W * gx * mp[0], sign[s] * W * gy * mp[1]]
        for g in range(n_groups):
            for a in range(3):
                hit = grp[:, a] == g + 1
                if not hit.any():
                    continue
                gterms[g].append((W * (gP[0] * G[:, a, 0] + gP[1] * G[:, a, 1]))[hit])
                for i in range(1, ns):
                    gterms[g].append((-W * coe * sign[i] * p.e[i] * phi[a])[hit])

    # ---- the walls ---------------------------------------------------------------------------------------------------
    tags = np.zeros((cells.shape[0], 3), dtype=np.int8) if tags is None else np.asarray(tags).reshape(-1, 3)
    wall = [[([], []) for _ in range(ns)] for _ in range(nt)]       # (terms, magnitudes)
    ionf = [([], []) for _ in range(nt)]
    ends = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
    for t in range(1, nt + 1):
        for i in range(3):
            cs = np.nonzero(tags[:, i] == t)[0]
            if cs.size == 0:
                continue
            j, kk = ends[i]
            sub = _Points(md, fields, U, cells[cs], G[cs])
            Gi = G[cs, i]
            gi = np.sqrt(Gi[:, 0] ** 2 + Gi[:, 1] ** 2)
            nx, ny = -Gi[:, 0] / gi, -Gi[:, 1] / gi
            e_ = x[cs, j] - x[cs, kk]
            L = np.sqrt(e_[:, 0] ** 2 + e_[:, 1] ** 2)
            for tq, w in zip(*fqp):
                phi = np.zeros(3)
                phi[j], phi[kk] = 1.0 - tq, tq
                W = w * L * two_pi * (rn[cs] @ phi)
                p = sub.at(phi)
                En = p.Ex * nx + p.Ey * ny
                ion, ion_mag = np.zeros(cs.size), np.zeros(cs.size)
                for s in range(1, ns):
                    if not int(md.is_ion[s]):
                        continue
                    add = [gx * nx + gy * ny for gx, gy in sub.flux_addends(p, s)]
                    gn = sum(add)
                    ion = ion + np.maximum(gn, 0.0)
                    ion_mag = ion_mag + np.where(gn > 0.0, sum(np.abs(a) for a in add), 0.0)
                ionf[t - 1][0].append(W * ion)
                ionf[t - 1][1].append(W * ion_mag)
                vth_e = np.sqrt(float(md.vth_e_coef) * p.me)
                for c in range(ns):
                    sp = ie if c == 0 else c
                    et = int(md.eq_type[sp])
                    if et == REACTION:
                        continue
                    ref = float(md.ref[t - 1][sp])
                    fac = (1.0 - ref) / (1.0 + ref)
                    vth = vth_e if sp == ie else float(md.vth[sp])
                    mu_scale, gam = 1.0, float(md.gamma[t - 1])
                    if c == 0:
                        vth, mu_scale, gam = vth * 1.3333, 5.0 / 3.0, gam * float(md.we_secondary)
                    dens = p.e[c]
                    parts = [W * fac * (0.5 * vth * dens)]
                    mags = [parts[0]]
                    if et != DIFFUSION_REACTION:
                        parts.append(W * fac * (np.abs(sign[sp] * mu_scale * p.mu[sp] * En) * dens))
                        mags.append(parts[-1])
                        if sp == ie:
                            parts.append(-W * (2.0 * gam / (1.0 + ref)) * ion)
                            mags.append(W * (2.0 * gam / (1.0 + ref)) * ion_mag)
                    wall[t - 1][c][0].extend(parts)
                    wall[t - 1][c][1].extend(mags)

    cen = (x[:, 0] + x[:, 1] + x[:, 2]) / 3.0
    Em = np.sqrt(gP[0] * gP[0] + gP[1] * gP[1])
    nodal = [_max(U[:, c]) for c in range(ns)] + [_max(U[:, 0] - U[:, ie])]
    return dict(content=[_sum(t) for t in content], rate_of_change=[_sum(t) for t in rate],
                reaction=[_sum(t) for t in reac], collision_loss=_sum(loss), joule=_sum(joule),
                wall=[[_sum(*wall[t][c]) for c in range(ns)] for t in range(nt)],
                ion_flux=[_sum(*ionf[t]) for t in range(nt)], induced_current=_sum(cur),
                group_sum=[_sum(t) for t in gterms], field=_max(Em, cen), nodal=nodal,
                net=np.array([[int(md.net[j][i]) for i in range(ns)] for j in range(nr)]))


def combine(sums, weights=None):
    """A signed combination of Sums: Sum(fsum of w value, sum of |w| abs, the plain values combined the same way)."""
    weights = [1.0] * len(sums) if weights is None else list(weights)
    return Sum(math.fsum(w * s.value for w, s in zip(weights, sums)), math.fsum(abs(w) * s.abs for w, s in zip(weights, sums)),
               float(sum(w * s.plain for w, s in zip(weights, sums))))


def imbalance(ref):
    """[ns] Sums of rate_of_change - source + sum_t wall, the sources formed as the caller of fedm_gd_balance forms them."""
    ns, nr = len(ref["content"]), len(ref["reaction"])
    out = []
    for c in range(ns):
        sums, w = [ref["rate_of_change"][c]], [1.0]
        if c == 0:
            sums += [ref["joule"], ref["collision_loss"]]
            w += [-1.0, 1.0]
        else:
            for j in range(nr):
                if ref["net"][j, c]:
                    sums.append(ref["reaction"][j])
                    w.append(-float(ref["net"][j, c]))
        for t in range(len(ref["wall"])):
            sums.append(ref["wall"][t][c])
            w.append(1.0)
        out.append(combine(sums, w))
    return out
