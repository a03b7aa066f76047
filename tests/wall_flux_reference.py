"""'flux source' walls for the oracle's LFA model and the wall models of the wall-flux tests (helper module).

oracle/forms.py's LFAModel assembles its boundary terms in one method, ``_boundary``; the subclass here calls it and then
adds, in numpy, the wall term of fedm/functions.py:514-522 with the LFA path's cell-constant coefficients:

    fac = (1 - ref) / (1 + ref)
    diffusion-reaction:        g = fac * 0.5 vth * n_s
    drift-diffusion-reaction:  g = fac * (0.5 vth + |Z_s mu_s(|E|) E.n|) * n_s
                               if emits[s]:  g -= 2 gamma / (1 + ref) * sum_{i: is_ion} max(Gamma_i.n, 0)
    R[a][s] += 2 pi r_q w_q L phi_a g,        Gamma_i.n = -D_i(|E|) grad(n_i).n + Z_i mu_i(|E|) E.n n_i

n = exp(u), grad n = n grad u (logarithmic) or n = u (linear).  The Jacobian is the exact derivative with
d|x| = sign(x), sign(0) = 1, and max(x, 0) = (x + |x|) / 2.  oracle.newton.newton_solve takes the model unchanged.
"""
import numpy as np

from oracle.forms import DRIFT_DIFFUSION_REACTION, REACTION, LFAModel
from oracle.quadrature import interval_rule

ENDS = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
VTH_ION, VTH_E = 4e2, 1e5
MU_ION, D_ION = 2e-4, 3e-6


class WallLFAModel(LFAModel):
    """LFAModel whose bc_type may hold 'flux source'; ``walls`` = dict(vth[tag-1][s], ref[tag-1][s], gamma[tag-1],
    emits[s], is_ion[s])."""

    def __init__(self, *args, walls, **kw):
        super().__init__(*args, **kw)
        self.walls = {k: np.asarray(v, dtype=float if k in ("vth", "ref", "gamma") else bool) for k, v in walls.items()}

    def _boundary(self, Uc, E, Em, dEm, mu, Re, Ke):
        super()._boundary(Uc, E, Em, dEm, mu, Re, Ke)
        for f in self.wall_facets():
            self._wall(f, Uc, E, Em, dEm, mu, Re, Ke)

    def wall_facets(self):
        """One record per (local facet, species) with 'flux source' entries: cells, 0-based tags, geometry."""
        out = []
        for i in range(3):
            tagged = np.nonzero(self.facet_tags[:, i] > 0)[0]
            for s in range(self.ns):
                if self.eq_type[s] == REACTION or tagged.size == 0:
                    continue
                kinds = np.array([self.bc_type[t - 1][s] == "flux source" for t in self.facet_tags[tagged, i]])
                if not kinds.any():
                    continue
                c = tagged[kinds]
                Gi = self.G[c, i]
                nrm = -Gi / np.linalg.norm(Gi, axis=1)[:, None]
                j, k = ENDS[i]
                out.append(dict(i=i, j=j, k=k, s=s, c=c, tag=self.facet_tags[c, i].astype(int) - 1, nrm=nrm,
                                L=np.linalg.norm(self.xc[c, j] - self.xc[c, k], axis=1),
                                gbn=np.einsum("cbd,cd->cb", self.G[c], nrm)))
        return out

    def _field_drift(self, s):
        return self.eq_type[s] == DRIFT_DIFFUSION_REACTION and self.drift_w[s] is None

    def ion_normal_flux(self, f, i2, Uc, E, Em, mu, phi):
        """Gamma_i.n of ion i2 at the facet point phi: (n, dn, grad(n).n, grad(u).n, diffusion part, drift part)."""
        c = f["c"]
        Dv = self.D[i2](Em)[0][c]
        zm = self.Z[i2] * mu[i2][0][c] if self._field_drift(i2) else np.zeros(c.size)
        En = np.einsum("cd,cd->c", E[c], f["nrm"])
        gun = np.einsum("cb,cb->c", Uc[c, :, i2], f["gbn"])
        n, dn = self._dens(Uc[c, :, i2] @ phi)
        gnn = n * gun if self.log else gun
        return n, dn, gnn, gun, -Dv * gnn, zm * En * n

    def _wall(self, f, Uc, E, Em, dEm, mu, Re, Ke):
        w_ = self.walls
        c, s, j, k, tg, gbn, L = f["c"], f["s"], f["j"], f["k"], f["tag"], f["gbn"], f["L"]
        iphi = self.neq - 1
        tq, wt = interval_rule(self.qdeg_facet)
        En = np.einsum("cd,cd->c", E[c], f["nrm"])
        ref, vth, gam = w_["ref"][tg, s], w_["vth"][tg, s], w_["gamma"][tg]
        fac = (1.0 - ref) / (1.0 + ref)
        drift = self._field_drift(s)
        absa, dabsa = np.zeros(c.size), np.zeros((c.size, 3))
        if drift:
            muv, mud = mu[s][0][c], mu[s][1][c]
            a = self.Z[s] * muv * En
            sg = np.where(a < 0.0, -1.0, 1.0)
            absa = sg * a
            dabsa = (sg * self.Z[s])[:, None] * ((mud * En)[:, None] * dEm[c] - muv[:, None] * gbn)
        cs = fac * (0.5 * vth + absa)
        emitting = drift and bool(w_["emits"][s])
        ions = [i2 for i2 in range(self.ns) if w_["is_ion"][i2] and self.eq_type[i2] != REACTION] if emitting else []
        ce = -2.0 * gam / (1.0 + ref)
        for t, w in zip(tq, wt):
            phi = np.zeros(3)
            phi[j], phi[k] = 1.0 - t, t
            W = w * L * 2.0 * np.pi * (self.rnod[c] @ phi)
            n, dn = self._dens(Uc[c, :, s] @ phi)
            for a in (j, k):
                Re[c, a, s] += W * cs * n * phi[a]
                if Ke is None:
                    continue
                for b in range(3):
                    Ke[c, a, s, b, s] += W * cs * dn * phi[a] * phi[b]
                    Ke[c, a, s, b, iphi] += W * fac * dabsa[:, b] * n * phi[a]
            for i2 in ions:
                ni, dni, gnn, gun, diff, drf = self.ion_normal_flux(f, i2, Uc, E, Em, mu, phi)
                Gn = diff + drf
                h = np.where(Gn < 0.0, 0.0, 1.0)
                Dv, Dd = (v[c] for v in self.D[i2](Em))
                zm, zd = ((self.Z[i2] * v[c] for v in mu[i2]) if self._field_drift(i2) else (np.zeros(c.size),) * 2)
                for a in (j, k):
                    Re[c, a, s] += W * ce * h * Gn * phi[a]
                    if Ke is None:
                        continue
                    for b in range(3):
                        dgnn = dni * phi[b] * gun + ni * gbn[:, b] if self.log else gbn[:, b]
                        Ke[c, a, s, b, i2] += W * ce * h * (-Dv * dgnn + zm * En * dni * phi[b]) * phi[a]
                        Ke[c, a, s, b, iphi] += W * ce * h * phi[a] * (
                            -Dd * dEm[c, b] * gnn + (zd * dEm[c, b] * En - zm * gbn[:, b]) * ni)

    def diagnostics(self, U):
        """What the preconditions of a comparison are asserted on: per wall facet its tag (1-based), E.n and |E|; per
        emitting facet point the diffusion and drift parts of every ion's Gamma.n."""
        Uc, E, Em = self.cell_fields(U)
        mu = [m(Em) for m in self.mu]
        tq, _ = interval_rule(self.qdeg_facet)
        facets, ion_points, seen = [], [], set()
        for f in self.wall_facets():
            En = np.einsum("cd,cd->c", E[f["c"]], f["nrm"])
            for m_, cell in enumerate(f["c"]):
                if (cell, f["i"]) not in seen:
                    seen.add((cell, f["i"]))
                    facets.append((int(f["tag"][m_]) + 1, float(En[m_]), float(Em[cell]), int(cell)))
            if not (self._field_drift(f["s"]) and self.walls["emits"][f["s"]]):
                continue
            for i2 in range(self.ns):
                if not self.walls["is_ion"][i2] or self.eq_type[i2] == REACTION:
                    continue
                for t in tq:
                    phi = np.zeros(3)
                    phi[f["j"]], phi[f["k"]] = 1.0 - t, t
                    _, _, _, _, diff, drf = self.ion_normal_flux(f, i2, Uc, E, Em, mu, phi)
                    ion_points += [(int(tg) + 1, float(a), float(b)) for tg, a, b in zip(f["tag"], diff, drf)]
        return facets, ion_points


# ---- the models of the tests ----------------------------------------------------------------------------------------
# species 0: ions (drift-diffusion, Z = +1, mu = 2e-4, D = 3e-6); species 1: the deck's electrons with its ionisation.
# The deck's boundary list (cases/streamer.py, BOUNDARIES = ['line', z1, z2, r1, r2]) numbers z = 0 as tag 1, z = BOX as
# tag 2, the axis as tag 3 and r = BOX as tag 4: the electrodes are the walls (the cathode z = 0 reflects and emits),
# r = BOX keeps the deck's Neumann condition for the electrons so that both facet terms run in one kernel, the axis is
# zero flux.
CATHODE, ANODE, AXIS, OUTER = 1, 2, 3, 4
WALL_BC = [["flux source", "flux source"], ["flux source", "flux source"], ["zero flux", "zero flux"], ["zero flux", "Neumann"]]


def two_species_walls(gamma_cathode=0.07):
    return dict(vth=[[VTH_ION, VTH_E], [VTH_ION, VTH_E], [0.0, 0.0], [0.0, 0.0]],
                ref=[[0.3, 0.3], [0.0, 0.0], [1.0, 1.0], [1.0, 1.0]], gamma=[gamma_cathode, 0.0, 0.0, 0.0],
                emits=[False, True], is_ion=[True, False])


def oracle_two_species(mesh, gamma_cathode=0.07, log=True, mu_e=None, D_e=None, k_ion=None):
    from oracle import streamer as ost
    from oracle.mesh import mark_boundaries
    om = WallLFAModel(mesh, 2, True, ["drift-diffusion-reaction", "drift-diffusion-reaction"], [1.0, -1.0],
                      mu=[MU_ION, ost.MU_E if mu_e is None else mu_e], D=[D_ION, ost.D_E if D_e is None else D_e],
                      reactions=[(ost.K_ION if k_ion is None else k_ion, [0, 1], [1, 1])],
                      facet_tags=mark_boundaries(mesh, ost.BOUNDARIES), bc_type=WALL_BC, qdeg=2, log_representation=log,
                      walls=two_species_walls(gamma_cathode))
    return om


def device_two_species_model(gamma_cathode=0.07, log=True, mu_e=None, D_e=None, k_ion=None):
    from fedm_amd.cases import streamer
    from fedm_amd.device import Model, Reaction, Walls
    from fedm_amd.termsum import TermSum, parse
    mu = parse(streamer.MU_E) if mu_e is None else mu_e
    rate = parse(streamer.ALPHA) * parse(streamer.MU_E) * TermSum.field() if k_ion is None else k_ion
    return Model(n_species=2, poisson=True, eq_type=["drift-diffusion-reaction", "drift-diffusion-reaction"],
                 Z=[1.0, -1.0], mu=[TermSum.const(MU_ION), mu],
                 D=[TermSum.const(D_ION), parse(streamer.D_E) if D_e is None else D_e],
                 reactions=[Reaction(rate, power=[0, 1], net=[1, 1])], bc_kind=WALL_BC, quadrature_degree=2,
                 log_representation=log, walls=Walls(**two_species_walls(gamma_cathode)))


def device_problem(coords, cells, model, reorder=True):
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem
    from fedm_amd.mesh import Marking_boundaries, Mesh
    msh = Mesh(coords, cells)
    dofs, vals = streamer.dirichlet(msh.coords)
    dofs = (dofs // 3) * model.n_eq + model.n_eq - 1
    return DeviceProblem(msh.coords, msh.cells, model, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                         dirichlet_dofs=dofs.astype(np.int32), dirichlet_vals=vals, reorder=reorder)


def set_dirichlet(om, coords):
    from fedm_amd.cases import streamer
    dofs, vals = streamer.dirichlet(np.asarray(coords))
    om.set_dirichlet((dofs // 3).astype(np.int64) * om.neq + om.neq - 1, vals)
    return om


# four species (tests/lfa_models.py): metastable (diffusion-reaction: the thermal term alone), ion, negative ion with a
# constant drift velocity (kept at zero flux), electrons
FOUR_BC = [["flux source", "flux source", "zero flux", "flux source"], ["flux source", "flux source", "zero flux", "flux source"],
           ["zero flux"] * 4, ["zero flux"] * 3 + ["Neumann"]]


def four_species_walls():
    v = [3e2, VTH_ION, 0.0, VTH_E]
    return dict(vth=[v, v, [0.0] * 4, [0.0] * 4], ref=[[0.3] * 4, [0.0] * 4, [1.0] * 4, [1.0] * 4],
                gamma=[0.07, 0.0, 0.0, 0.0], emits=[False, False, False, True], is_ion=[False, True, False, False])


def four_species_pair():
    """(mesh, device Model, oracle WallLFAModel, Dirichlet dofs, values) of lfa_models.four_species_problem with walls."""
    from fedm_amd.device import Walls
    from lfa_models import four_species_problem
    m, prob, om0, ddofs, dvals = four_species_problem()
    model = prob.model
    prob.close()
    model.bc_kind = FOUR_BC
    model.walls = Walls(**four_species_walls())
    om = WallLFAModel(om0.mesh, 4, True, om0.eq_type, om0.Z, mu=om0.mu, D=om0.D, drift_w=om0.drift_w,
                      reactions=om0.reactions, facet_tags=om0.facet_tags, bc_type=FOUR_BC, qdeg=2,
                      walls=four_species_walls())
    om.dirichlet_dofs, om.dirichlet_vals = om0.dirichlet_dofs, om0.dirichlet_vals
    return m, model, om, ddofs, dvals


def wall_state(coords, neq=3, log=True):
    """The streamer's initial log densities plus a smooth perturbation, and the potential of the issue:
    V0 (z + 3 sin(3 pi r + 0.4) z (1 - z) + 0.4 sin(2.5 pi z + 0.3) r^2), r and z in units of the box."""
    from fedm_amd.cases import streamer
    coords = np.asarray(coords)
    r, z = coords[:, 0] / streamer.BOX, coords[:, 1] / streamer.BOX
    u_ion, u_e = streamer.initial_log_densities(coords)
    U = np.zeros((coords.shape[0], neq))
    U[:, 0] = u_ion + 0.4 * np.sin(5.0 * r + 1.0) * np.cos(4.0 * z)
    U[:, neq - 2] = u_e + 0.5 * np.cos(3.0 * r) * np.sin(6.0 * z + 0.5)
    if neq == 5:                 # metastable, ion, negative ion, electrons
        U[:, 0] = 27.0 + np.sin(4 * r) * np.cos(2 * z)
        U[:, 1] = u_ion + 0.4 * np.sin(5.0 * r + 1.0) * np.cos(4.0 * z)
        U[:, 2] = 25.0 + np.sin(3 * r + 2 * z)
    if not log:
        U[:, :neq - 1] = np.exp(U[:, :neq - 1])
    U[:, neq - 1] = streamer.U_W * (z + 3.0 * np.sin(3.0 * np.pi * r + 0.4) * z * (1.0 - z)
                                    + 0.4 * np.sin(2.5 * np.pi * z + 0.3) * r ** 2)
    return U


def assert_preconditions(om, U, emitting_tag=CATHODE):
    """Both signs of E.n on every 'flux source' tag, both signs of Gamma_ion.n on the emitting tag, and no facet or
    facet point within 1e-6 relative of a kink: there two correct implementations may pick different one-sided
    derivatives.  Asserted on the restatement's numbers; nothing is filtered."""
    facets, ion_points = om.diagnostics(U)
    tags = sorted({t for t, *_ in facets})
    for t in tags:
        En = np.array([e for tt, e, *_ in facets if tt == t])
        assert (En > 0).any() and (En < 0).any(), (t, En)
    ratio = min(abs(e) / em for _, e, em, _ in facets)
    assert ratio > 1e-6, ratio
    g = np.array([a + b for t, a, b in ion_points if t == emitting_tag])
    assert (g > 0).any() and (g < 0).any()
    kink = min(abs(a + b) / (abs(a) + abs(b)) for _, a, b in ion_points)
    assert kink > 1e-6, kink
    return dict(tags=tags, min_En_over_E=ratio, min_ion_kink=kink, n_facets=len(facets))
