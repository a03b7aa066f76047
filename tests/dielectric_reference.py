"""Dielectric layers for the wall-flux restatement (helper module): numpy only, nothing shared with the device.

A boundary tag T may be a layer of thickness d and relative permittivity eps_r with a conductor at voltage U behind it.
Per vertex a of a layer the model keeps q_a = int sigma phi_a 2 pi r ds and its predecessor.  W_a,s(u) is what the
boundary terms of wall_flux_reference.WallLFAModel (and of the oracle's Neumann term) add to residual entry (a, s) on
the layer's facets; with w = dt/dt_old

    q_a(u) = [(1 + w)^2 q_a - w^2 q_old_a]/(1 + 2w) + dt (1 + w)/(1 + 2w) e sum_s Z_s W_a,s(u)
    R_Phi,a += sum_q W_q (eps_r/d)(Phi_q - U) phi_a - q_a(u)/eps0

The Jacobian is analytic: the Robin mass term, and every boundary entry of a species row on a layer facet once more
in the Poisson row times -kappa Z_s, kappa = (e/eps0) dt (1 + w)/(1 + 2w); tests/test_dielectric_reference.py checks
it against finite differences.

``fault`` builds one deliberate error in, for the tests that show the GPU bounds would catch it.
"""
import numpy as np
import scipy.sparse as sp

import wall_flux_reference as wr
from oracle.forms import elementary_charge, epsilon_0
from oracle.quadrature import interval_rule

FAULTS = ("Z dropped from the mirror", "history left out", "w^2 taken as w", "potential column not mirrored",
          "Robin term without U", "emission not deposited")


class DielectricLFAModel(wr.WallLFAModel):
    """WallLFAModel with ``layers`` = {tag: (d, eps_r, U)} (tags from 1) and the charge moments ``q``, ``q_old`` per
    vertex (zero off the layers)."""

    def __init__(self, *args, layers, fault=None, **kw):
        super().__init__(*args, **kw)
        assert fault is None or fault in FAULTS
        self.layers = {int(t): tuple(float(x) for x in v) for t, v in layers.items()}
        self.fault = fault
        self.q = np.zeros(self.mesh.nv)
        self.q_old = np.zeros(self.mesh.nv)
        self._step = None
        self._layer_R = None
        on = np.isin(self.facet_tags, list(self.layers))
        self.layer_vertices = np.unique(np.concatenate(
            [self.mesh.cells[np.nonzero(on[:, i])[0]][:, list(wr.ENDS[i])].ravel() for i in range(3)]).astype(np.int64))

    # -- time coefficients ----------------------------------------------------------------------------------------------
    def step_coefficients(self, dt, dt_old):
        """(a1, a2, cdt): q(u) = a1 q - a2 q_old + cdt e sum_s Z_s W_s(u)"""
        w = dt / dt_old
        w2 = w if self.fault == "w^2 taken as w" else w * w
        return (1.0 + w) ** 2 / (1.0 + 2.0 * w), w2 / (1.0 + 2.0 * w), dt * (1.0 + w) / (1.0 + 2.0 * w)

    def history(self, dt, dt_old):
        a1, a2, _ = self.step_coefficients(dt, dt_old)
        if self.fault == "history left out":
            return np.zeros_like(self.q)
        return a1 * self.q - a2 * self.q_old

    # -- the boundary terms, the layer's apart ----------------------------------------------------------------------------
    def element_tensors(self, U, Uold, Uold1, dt, dt_old, jacobian=True):
        self._step = (dt, dt_old)
        return super().element_tensors(U, Uold, Uold1, dt, dt_old, jacobian)

    def _boundary_of(self, tags, Uc, E, Em, dEm, mu, Re, Ke, gamma=None):
        keep, keep_gamma = self.facet_tags, self.walls["gamma"]
        self.facet_tags = tags
        if gamma is not None:
            self.walls["gamma"] = gamma
        try:
            super()._boundary(Uc, E, Em, dEm, mu, Re, Ke)
        finally:
            self.facet_tags, self.walls["gamma"] = keep, keep_gamma

    def _boundary(self, Uc, E, Em, dEm, mu, Re, Ke):
        tags = self.facet_tags
        on = np.isin(tags, list(self.layers))
        Rl = np.zeros_like(Re)
        Kl = None if Ke is None else np.zeros_like(Ke)
        self._boundary_of(np.where(on, 0, tags), Uc, E, Em, dEm, mu, Re, Ke)
        self._boundary_of(np.where(on, tags, 0), Uc, E, Em, dEm, mu, Rl, Kl)
        Re += Rl
        if Ke is not None:
            Ke += Kl
        if self.fault == "emission not deposited":     # the mirror sees the walls without their secondaries
            Rl = np.zeros_like(Re)
            Kl = None if Ke is None else np.zeros_like(Ke)
            self._boundary_of(np.where(on, tags, 0), Uc, E, Em, dEm, mu, Rl, Kl, gamma=np.zeros_like(self.walls["gamma"]))
        self._layer_R = Rl
        iphi = self.neq - 1
        kappa = elementary_charge / epsilon_0 * self.step_coefficients(*self._step)[2]
        for s in range(self.ns):
            z = 1.0 if self.fault == "Z dropped from the mirror" else self.Z[s]
            Re[:, :, iphi] -= kappa * z * Rl[:, :, s]
            if Ke is None:
                continue
            cols = slice(0, iphi) if self.fault == "potential column not mirrored" else slice(None)
            Ke[:, :, iphi, :, cols] -= kappa * z * Kl[:, :, s, :, cols]
        self._robin(Uc, Re, Ke)

    def _robin(self, Uc, Re, Ke):
        iphi = self.neq - 1
        tq, wt = interval_rule(self.qdeg_facet)
        for i in range(3):
            j, k = wr.ENDS[i]
            for tag, (d, eps_r, U) in self.layers.items():
                c = np.nonzero(self.facet_tags[:, i] == tag)[0]
                if c.size == 0:
                    continue
                L = np.linalg.norm(self.xc[c, j] - self.xc[c, k], axis=1)
                if self.fault == "Robin term without U":
                    U = 0.0
                for t, w in zip(tq, wt):
                    phi = np.zeros(3)
                    phi[j], phi[k] = 1.0 - t, t
                    W = w * L * 2.0 * np.pi * (self.rnod[c] @ phi) * eps_r / d
                    dphi = Uc[c, :, iphi] @ phi - U
                    for a in (j, k):
                        Re[c, a, iphi] += W * dphi * phi[a]
                        if Ke is None:
                            continue
                        for b in (j, k):
                            Ke[c, a, iphi, b, iphi] += W * phi[a] * phi[b]

    def robin_matrix(self):
        """(eps_r/d) int phi_a phi_b 2 pi r ds over the layers' facets, vertex by vertex: the constant part of the
        (Phi, Phi) block that the layers add"""
        nc, neq = self.mesh.nc, self.neq
        Ke = np.zeros((nc, 3, neq, 3, neq))
        self._robin(np.zeros((nc, 3, neq)), np.zeros((nc, 3, neq)), Ke)
        c = self.mesh.cells.astype(np.int64)
        rows = np.broadcast_to(c[:, :, None], (nc, 3, 3)).ravel()
        cols = np.broadcast_to(c[:, None, :], (nc, 3, 3)).ravel()
        return sp.coo_matrix((Ke[:, :, neq - 1, :, neq - 1].ravel(), (rows, cols)), shape=(self.mesh.nv,) * 2).tocsr()

    # -- residual and Jacobian with the history in the Poisson rows --------------------------------------------------------
    def _with_history(self, F, U, dt, dt_old, apply_bc):
        iphi = self.neq - 1
        F[self.layer_vertices * self.neq + iphi] -= self.history(dt, dt_old)[self.layer_vertices] / epsilon_0
        if apply_bc and self.dirichlet_dofs.size:
            F[self.dirichlet_dofs] = U.ravel()[self.dirichlet_dofs] - self.dirichlet_vals
        return F

    def residual(self, U, Uold, Uold1, dt, dt_old, apply_bc=True):
        F = super().residual(U, Uold, Uold1, dt, dt_old, apply_bc=False)
        return self._with_history(F, U, dt, dt_old, apply_bc)

    def residual_jacobian(self, U, Uold, Uold1, dt, dt_old, apply_bc=True):
        F, J = super().residual_jacobian(U, Uold, Uold1, dt, dt_old, apply_bc=False)
        F = self._with_history(F, U, dt, dt_old, apply_bc)
        if apply_bc and self.dirichlet_dofs.size:
            J = self._dirichlet_rows(J)
        return F, J

    # -- the charge ----------------------------------------------------------------------------------------------------------
    def wall_moments(self, U, dt, dt_old):
        """sum_s Z_s W_a,s(u) per vertex (zero off the layers), from the boundary terms of the layer's facets."""
        self.element_tensors(U, U, U, dt, dt_old, jacobian=False)
        out = np.zeros(self.mesh.nv)
        for s in range(self.ns):
            np.add.at(out, self.mesh.cells.ravel(), self.Z[s] * self._layer_R[:, :, s].ravel())
        return out

    def charge(self, U, dt, dt_old):
        """q_a(u)"""
        _, _, cdt = self.step_coefficients(dt, dt_old)
        return self.history(dt, dt_old) + cdt * elementary_charge * self.wall_moments(U, dt, dt_old)

    def accept(self, U, dt, dt_old):
        q = self.charge(U, dt, dt_old)
        self.q_old, self.q = self.q, q

    def species_charge(self, U):
        """e sum_s Z_s N_s with the time term's quadrature"""
        from oracle.lagrange import p1_basis
        from oracle.quadrature import triangle_rule
        Uc = U[self.mesh.cells]
        xq, wq = triangle_rule(self.qdeg_time)
        total = 0.0
        for xi, w in zip(xq, wq):
            phi = p1_basis(xi[None, :])[0]
            W = w * self.detJ * 2.0 * np.pi * (self.rnod @ phi)
            for s in range(self.ns):
                total += elementary_charge * self.Z[s] * float(np.sum(W * self._dens(Uc[:, :, s] @ phi)[0]))
        return total

    def displacement_charge(self, U):
        """eps0 eps_r/d int (Phi - U) 2 pi r ds per layer tag"""
        Uc = U[self.mesh.cells]
        tq, wt = interval_rule(self.qdeg_facet)
        out = {}
        for tag, (d, eps_r, Ut) in self.layers.items():
            tot = 0.0
            for i in range(3):
                j, k = wr.ENDS[i]
                c = np.nonzero(self.facet_tags[:, i] == tag)[0]
                L = np.linalg.norm(self.xc[c, j] - self.xc[c, k], axis=1)
                for t, w in zip(tq, wt):
                    phi = np.zeros(3)
                    phi[j], phi[k] = 1.0 - t, t
                    tot += float(np.sum(w * L * 2.0 * np.pi * (self.rnod[c] @ phi) * (Uc[c, :, self.neq - 1] @ phi - Ut)))
            out[tag] = epsilon_0 * eps_r / d * tot
        return out


# ---- the models of the tests --------------------------------------------------------------------------------------------
# Layer on the cathode (tag 1: both species 'flux source', the electrons with emission) or on r = BOX (tag 4: the
# electrons' Neumann term).  Thickness and permittivity of a glass-like coating; the conductor behind it at a voltage
# of some tens of volts.  wall_state's potential runs to kilovolts along both walls (it is made to give E.n both signs
# there), so the layer is a millimetre thick: (eps_r/d) (Phi - U) then stays within a few times the gap field, 1e6 V/m.
LAYER_D, LAYER_EPS_R, LAYER_U = 1e-3, 4.0, 30.0
CONFIGS = {"cathode": wr.CATHODE, "outer": wr.OUTER}


def layers_of(config):
    return {CONFIGS[config]: (LAYER_D, LAYER_EPS_R, LAYER_U)}


def dirichlet(coords, config, neq=3):
    """The streamer's electrode values on the potential -- without the electrode the layer covers: the conductor is
    behind the layer, at the layer's voltage.  "outer": both electrodes stay, and their corner vertices at r = BOX are
    on the layer and Dirichlet vertices at once."""
    from fedm_amd.cases import streamer
    dofs, vals = streamer.dirichlet(np.asarray(coords))
    if config == "cathode":
        keep = np.abs(np.asarray(coords)[dofs // 3, 1]) > 3e-16
        dofs, vals = dofs[keep], vals[keep]
    return (dofs // 3).astype(np.int64) * neq + neq - 1, vals


def device_problem(coords, cells, model, config, reorder=True):
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem
    from fedm_amd.mesh import Marking_boundaries, Mesh
    msh = Mesh(coords, cells)
    dofs, vals = dirichlet(msh.coords, config, model.n_eq)
    return DeviceProblem(msh.coords, msh.cells, model, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                         dirichlet_dofs=dofs.astype(np.int32), dirichlet_vals=vals, reorder=reorder)


def oracle_two_species(mesh, config, fault=None, bc_type=None, **kw):
    """wall_flux_reference.oracle_two_species with a layer and this module's Dirichlet values."""
    om = with_layers(wr.oracle_two_species(mesh, **kw), layers_of(config), fault=fault, bc_type=bc_type)
    om.set_dirichlet(*dirichlet(mesh.coords, config))
    return om


def with_layers(base, layers, fault=None, bc_type=None):
    """A WallLFAModel once more, with layers (its Dirichlet values are not taken over)."""
    return DielectricLFAModel(base.mesh, base.ns, True, base.eq_type, base.Z, mu=base.mu, D=base.D, drift_w=base.drift_w,
                              reactions=base.reactions, facet_tags=base.facet_tags,
                              bc_type=base.bc_type if bc_type is None else bc_type, qdeg=base.qdeg_facet,
                              axisymmetric=base.axisymmetric, log_representation=base.log,
                              walls={k: v.copy() for k, v in base.walls.items()}, layers=layers, fault=fault)


def device_two_species_model(config, **kw):
    from fedm_amd.device import Dielectric
    model = wr.device_two_species_model(**kw)
    tag = CONFIGS[config]
    model.dielectric = Dielectric(thickness={tag: LAYER_D}, eps_r={tag: LAYER_EPS_R}, voltage={tag: LAYER_U})
    return model


def random_history(om, seed=11, scale=2e-10):
    """Non-zero q and q_old on the layer vertices.  The scale is the charge that screens the gap field on a vertex's
    share of the wall of the 20 x 20 mesh (r ~ 6e-3 m, ds ~ 6e-4 m): eps0 * 1e6 V/m * 2 pi 6e-3 * 6e-4 ~ 2e-10 C."""
    rng = np.random.default_rng(seed)
    q, q_old = np.zeros(om.mesh.nv), np.zeros(om.mesh.nv)
    lv = om.layer_vertices
    q[lv] = scale * rng.normal(size=lv.size)
    q_old[lv] = scale * rng.normal(size=lv.size)
    return q, q_old
