"""Device context: the Python face of libfedm_hip.so.

One :class:`DeviceProblem` holds a mesh, a model descriptor and the state
vectors in HBM and offers what the reference reaches through DOLFIN:

* ``residual`` / ``jacobian``   <- ``Problem.F`` / ``Problem.J``  (fedm/functions.py:188-202)
* ``newton_solve``              <- ``PETScSNESSolver.solve``      (fedm/functions.py:1047)
* ``field_error``               <- the two ``df.norm`` calls      (fedm/functions.py:1062-1064)

Numerical failure (non-convergence, NaN) raises ``RuntimeError`` exactly where
DOLFIN's ``error_on_nonconvergence`` would, so ``adaptive_solver``'s catch-all
retry (fedm/functions.py:1080) keeps working.
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, quadrature
from .photo import Photoionization
from .physical_constants import elementary_charge, epsilon_0
from .termsum import TermSum


@dataclass
class Reaction:
    k: TermSum                 # rate coefficient as a function of |E|
    power: Sequence[int]       # power-matrix row over the solved species
    net: Sequence[int]         # gain - loss row


@dataclass
class Walls:
    """The 'flux source' walls of an LFA model (Boundary_flux, fedm/functions.py:514-522): thermal velocity and
    reflection coefficient per (tag, species), secondary emission coefficient per tag, the species that receives the
    secondary electrons and the ions whose wall flux releases them."""
    vth: Sequence[Sequence[float]]             # [tag-1][species]
    ref: Sequence[Sequence[float]]             # [tag-1][species]
    gamma: Sequence[float]                     # [tag-1]
    emits: Sequence[bool]                      # [species]
    is_ion: Sequence[bool]                     # [species]

    def to_c(self, n_species):
        wd = _lib.WallDesc()
        if not len(self.vth) == len(self.ref) == len(self.gamma) <= _lib.MAX_TAGS:
            raise ValueError(f"Walls: vth, ref and gamma need one entry per boundary tag, at most {_lib.MAX_TAGS}")
        for t in range(len(self.gamma)):
            wd.gamma[t] = float(self.gamma[t])
            for s in range(n_species):
                wd.vth[t][s], wd.ref[t][s] = float(self.vth[t][s]), float(self.ref[t][s])
        for s in range(n_species):
            wd.emits[s], wd.is_ion[s] = int(bool(self.emits[s])), int(bool(self.is_ion[s]))
        return wd


@dataclass
class Dielectric:
    """Dielectric layers on boundary tags of an LFA model (thin-layer approximation, ``fedm_ctx_create_dielectric``): per
    layer tag (as the mesh numbers it, from 1) the thickness [m], the relative permittivity and the voltage of the
    conductor behind it at the start (:meth:`DeviceProblem.set_layer_voltage` changes it)."""
    thickness: dict                            # {tag: d}
    eps_r: dict = field(default_factory=dict)  # {tag: eps_r}, 1 where missing
    voltage: dict = field(default_factory=dict)   # {tag: U}, 0 where missing

    def tags(self):
        return sorted(int(t) for t in self.thickness)

    def to_c(self):
        dd = _lib.DielectricDesc()
        for t in self.tags():
            if not 1 <= t <= _lib.MAX_TAGS:
                raise ValueError(f"Dielectric: tag {t} outside 1..{_lib.MAX_TAGS}")
            dd.is_layer[t - 1] = 1
            dd.thickness[t - 1] = float(self.thickness[t])
            dd.eps_r[t - 1] = float(self.eps_r.get(t, 1.0))
            dd.voltage[t - 1] = float(self.voltage.get(t, 0.0))
        return dd


@dataclass
class Model:
    """What fedm.functions' weak-form builders describe (see functions.py)."""
    n_species: int
    poisson: bool
    eq_type: Sequence[str]
    Z: Sequence[float]
    mu: Sequence[TermSum] = ()
    D: Sequence[TermSum] = ()
    drift_w: Sequence[Optional[Tuple[float, float]]] = ()
    reactions: Sequence[Reaction] = ()
    bc_kind: Sequence[Sequence[str]] = ()      # [tag-1][species]
    quadrature_degree: int = 2
    ext_source_degree: Sequence[int] = ()      # 0 = none, k = Expression(degree=k) source
    axisymmetric: bool = True
    log_representation: bool = True            # False: the unknowns are the densities (functions.py:350-368)
    walls: Optional[Walls] = None              # for the 'flux source' entries of bc_kind
    # Helmholtz photoionisation source (fedm_amd.photo): its targets get degree-1 source tables, which the device fills
    photoionization: Optional[Photoionization] = None
    dielectric: Optional[Dielectric] = None    # dielectric layers on boundary tags (None: the model as it was)

    @property
    def n_eq(self):
        return self.n_species + (1 if self.poisson else 0)

    def source_table_degrees(self):
        """``ext_source_degree`` with the degree-1 tables that ``photoionization`` implies on its targets."""
        ext = list(self.ext_source_degree) or [0] * self.n_species
        if self.photoionization is not None:
            self.photoionization.check(self)
            for s in self.photoionization.targets:
                if ext[s] not in (0, 1):
                    raise ValueError(f"species {s} receives the photoionisation source through a degree-1 source table; "
                                     f"it has an Expression source of degree {ext[s]}")
                ext[s] = 1
        return ext

    def walls_to_c(self):
        """fedm_wall_desc for fedm_ctx_create_walls, or None for a model without 'flux source' entries."""
        if not any(k == "flux source" for row in self.bc_kind for k in row):
            return None
        if self.walls is None:
            raise ValueError("a model with 'flux source' boundaries needs walls=Walls(...)")
        if len(self.walls.gamma) != len(self.bc_kind):
            raise ValueError(f"Walls describes {len(self.walls.gamma)} boundary tags, bc_kind {len(self.bc_kind)}")
        return self.walls.to_c(self.n_species)

    def to_c_tabulated(self):
        """The descriptor and the model's distinct coefficient tables as fedm_ctx_create_tabulated takes them:
        (md, tab_ptr int32[n_tables + 1], tab_x, tab_y).  Equal tables go in once."""
        tables = []
        md = self.to_c(tables)
        ptr = np.zeros(len(tables) + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([t.x.size for t in tables])
        if ptr[-1] > _lib.MAX_TABLE_KNOTS:
            raise ValueError(f"the model's coefficient tables have {ptr[-1]} knots in all, at most "
                             f"{_lib.MAX_TABLE_KNOTS}")
        cat = lambda arrs: np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros(0), dtype=np.float64)
        return md, ptr, cat([t.x for t in tables]), cat([t.y for t in tables])

    def to_c(self, tables=None):
        """The descriptor ALONE.  For a model with tabulated coefficients it holds their table references
        (``fedm_termsum.pad_``) but not the tables they index: ``tables`` is the list that collects those, and
        ``to_c_tabulated()`` -- which DeviceProblem calls -- returns both.  Called without a list the references are
        still written (the descriptor's bytes identify the model, which is what callers of this form compare);
        ``fedm_ctx_create`` refuses such a descriptor, so it cannot reach the device without its tables."""
        tables = [] if tables is None else tables
        md = _lib.ModelDesc()
        ns = self.n_species
        md.linear_representation = 0 if self.log_representation else 1
        if not 1 <= ns <= _lib.MAX_SPECIES:
            raise ValueError(f"n_species must be 1..{_lib.MAX_SPECIES}")
        md.n_species, md.poisson, md.axisymmetric = ns, int(self.poisson), int(self.axisymmetric)
        mu = list(self.mu) or [TermSum.const(0.0)] * ns
        D = list(self.D) or [TermSum.const(0.0)] * ns
        w = list(self.drift_w) or [None] * ns
        for s in range(ns):
            md.eq_type[s] = _lib.EQ_TYPES[self.eq_type[s]]
            md.Z[s] = float(self.Z[s])
            TermSum.coerce(mu[s]).fill(md.mu[s], tables)
            TermSum.coerce(D[s]).fill(md.D[s], tables)
            if w[s] is not None:
                md.has_drift_w[s] = 1
                md.drift_w[s][0], md.drift_w[s][1] = float(w[s][0]), float(w[s][1])
        if len(self.reactions) > _lib.MAX_REACTIONS:
            raise ValueError(f"at most {_lib.MAX_REACTIONS} reactions")
        md.n_reactions = len(self.reactions)
        for j, rc in enumerate(self.reactions):
            TermSum.coerce(rc.k).fill(md.k[j], tables)
            for s in range(ns):
                md.power[j][s] = int(rc.power[s])
                md.net[j][s] = int(rc.net[s])
        md.charge_over_eps = elementary_charge / epsilon_0
        md.n_tags = len(self.bc_kind)
        if md.n_tags > _lib.MAX_TAGS:
            raise ValueError(f"at most {_lib.MAX_TAGS} boundary tags")
        for t, row in enumerate(self.bc_kind):
            for s in range(ns):
                md.bc_kind[t][s] = _lib.BC_KINDS[row[s]]
        xq, wq = quadrature.triangle(self.quadrature_degree)
        if len(wq) > _lib.MAX_QP:
            raise ValueError("quadrature rule too large")
        md.n_qp = len(wq)
        for q in range(len(wq)):
            md.qp_x[q], md.qp_y[q], md.qp_w[q] = xq[q, 0], xq[q, 1], wq[q]
        tq, wt = quadrature.interval(self.quadrature_degree)
        md.n_fqp = len(wt)
        for q in range(len(wt)):
            md.fqp_t[q], md.fqp_w[q] = tq[q], wt[q]
        ext = self.source_table_degrees()
        degs = {k for k in ext if k}
        if len(degs) > 1:
            raise ValueError("all Expression sources must share one degree")
        for s in range(ns):
            md.ext_nodes[s] = (ext[s] + 1) * (ext[s] + 2) // 2 if ext[s] else 0
        if degs:
            B, _ = quadrature.lagrange_interpolation_matrix(degs.pop(), xq)
            for q in range(B.shape[0]):
                for m in range(B.shape[1]):
                    md.ext_B[q][m] = B[q, m]
        return md


@dataclass
class GdModel:
    """LMEA model family (examples/glow_discharge/fedm-gd.py): energy equation + particle
    balances with nodal, semi-implicit coefficients + Poisson.  Species 0 is the gas."""
    n_species: int
    N0: float
    eq_type: Sequence[str]
    grad_diffusion: Sequence[bool]
    is_ion: Sequence[bool]
    sign: Sequence[float]
    vth: Sequence[float]
    electron_mass: float
    power: Sequence[Sequence[int]]
    net: Sequence[Sequence[int]]
    energy_loss: Sequence[float]
    ref: Sequence[Sequence[float]]             # [tag-1][species]
    gamma: Sequence[float]                     # [tag-1]
    we_secondary: float
    quadrature_degree: int = 4
    axisymmetric: bool = True
    poisson: bool = True
    # Energy_Source_term's Ei and mean_energy (fedm/functions.py:855, 906-909) for the sentinel losses 7.77e77 / 9.99e99
    # left in `energy_loss`: None (no sentinel may be present) or "unknown_ratio" = u[0] / u[n - 1] (fedm-gd.py:358)
    energy_Ei: float = 0.0
    mean_energy_form: Optional[str] = None

    @property
    def n_eq(self):
        return self.n_species + 1

    @property
    def n_reactions(self):
        return len(self.power)

    @property
    def n_fields(self):
        return 4 * self.n_species + 2 * self.n_reactions + 3

    def to_c(self):
        md = _lib.GdDesc()
        ns, nr = self.n_species, self.n_reactions
        if ns > _lib.GD_MAX_SPECIES - 1 or nr > _lib.GD_MAX_REACTIONS or len(self.ref) > _lib.MAX_TAGS:
            raise ValueError("LMEA model too large for the device descriptor")
        md.n_species, md.n_reactions, md.n_tags = ns, nr, len(self.ref)
        md.axisymmetric, md.N0 = int(self.axisymmetric), float(self.N0)
        md.charge_over_eps = elementary_charge / epsilon_0
        for i in range(ns):
            md.eq_type[i] = _lib.EQ_TYPES[self.eq_type[i]]
            md.grad_diffusion[i] = int(bool(self.grad_diffusion[i]))
            md.is_ion[i] = int(bool(self.is_ion[i]))
            md.sign[i] = float(self.sign[i])
            md.vth[i] = float(self.vth[i])
        md.vth_e_coef = 16.0 * elementary_charge / (3.0 * np.pi * self.electron_mass)
        for j in range(nr):
            md.energy_loss[j] = float(self.energy_loss[j])
            for i in range(ns):
                md.power[j][i] = int(self.power[j][i])
                md.net[j][i] = int(self.net[j][i])
        for t in range(len(self.ref)):
            md.gamma[t] = float(self.gamma[t])
            for i in range(ns):
                md.ref[t][i] = float(self.ref[t][i])
        md.we_secondary = float(self.we_secondary)
        sentinel = any(7e77 < v < 8e77 or 9e99 < v < 1e100 for v in self.energy_loss)
        if sentinel and self.mean_energy_form is None:
            raise ValueError("energy losses that depend on the mean energy need mean_energy_form")
        md.energy_Ei = float(self.energy_Ei)
        md.mean_energy_form = _lib.GD_ME_FORMS[self.mean_energy_form]
        xq, wq = quadrature.triangle(self.quadrature_degree)
        md.n_qp = len(wq)
        for q in range(len(wq)):
            md.qp_x[q], md.qp_y[q], md.qp_w[q] = xq[q, 0], xq[q, 1], wq[q]
        tq, wt = quadrature.interval(self.quadrature_degree)
        md.n_fqp = len(wt)
        for q in range(len(wt)):
            md.fqp_t[q], md.fqp_w[q] = tq[q], wt[q]
        return md


@dataclass
class NewtonReport:
    iterations: int
    converged: bool
    linear_iterations: int
    fnorm0: float
    fnorm: float


@dataclass
class Diagnostics:
    """One call of :meth:`DeviceProblem.diagnostics` (``fedm_diagnostics``, include/fedm_hip.h has the formulae).
    Indices in the caller's numbering, -1 where there is none; lengths in m."""
    species_integral: np.ndarray      # N_s = int n_s (2 pi r) dx per species: particles, or per metre of depth (planar)
    group_sum: np.ndarray             # q_g: the unconstrained Poisson rows summed over vertex group g  [V m]
    induced_current: float            # I_psi = sum_s Z_s int Gamma_s . (-grad psi)  [1/s]; 0 without a psi
    field_max: float                  # max over the cells of |grad Phi|  [V/m]
    field_max_cell: int
    field_max_centroid: Tuple[float, float]
    window_max: float                 # the same over the cells whose centroid lies in the window
    window_max_cell: int
    window_max_centroid: Tuple[float, float]
    nodal_max: np.ndarray             # max_v u_s(v): bitwise a value of the state (ln n_s, or n_s when linear)
    nodal_max_vertex: np.ndarray
    finite: bool                      # False: a value met on the way was not finite; the rest is unspecified
    Z: np.ndarray                     # the species' charge numbers
    linear_representation: bool = False

    @property
    def net_charge(self):
        """sum_s Z_s N_s in elementary charges."""
        return float(np.dot(self.Z, self.species_integral))

    @property
    def surface_charge(self):
        """eps0 q_g [C; C/m planar]: the charge on electrode g, BoundaryGradient in integrated form."""
        return epsilon_0 * self.group_sum

    @property
    def current(self):
        """e I_psi [A; A/m planar]."""
        return elementary_charge * self.induced_current

    @property
    def density_max(self):
        """the densities at the nodal maxima."""
        return self.nodal_max.copy() if self.linear_representation else np.exp(self.nodal_max)

    @property
    def z_head(self):
        """z of the window's field maximum: the head position when the window is the channel."""
        return self.window_max_centroid[1]


@dataclass
class Balance:
    """One call of :meth:`DeviceProblem.balance` (``fedm_gd_balance``, include/fedm_hip.h has the formulae): the particle
    and energy balance of an LMEA model at the state the residual of the current step sees.  Component 0 is the energy
    equation, 1..ns-1 the species (the last the electrons).  Axisymmetric: totals; planar: per metre of depth.  Indices in
    the caller's numbering (on an exact tie of the field maximum the lowest cell in the device's order)."""
    content: np.ndarray               # [ns] int exp(u_c): particles; [0] the electrons' energy [eV]
    rate_of_change: np.ndarray        # [ns] int of the residual's BDF2 term  [1/s; eV/s]
    reaction: np.ndarray              # [nr] int R_j  [1/s]
    collision_loss: float             # int sum_j loss_j R_j  [eV/s]
    joule: float                      # int -Gamma_e . E  [eV/s]
    wall: np.ndarray                  # [n_tags, ns] the walls' facet integrals of row c, per boundary tag
    ion_flux: np.ndarray              # [n_tags] int sum_ions max(Gamma_i . n, 0)  [1/s]
    induced_current: float            # sum_s sign_s int Gamma_s . (-grad psi)  [1/s]; 0 without a psi
    group_sum: np.ndarray             # the unconstrained Poisson rows summed over vertex group g  [V m]
    field_max: float                  # max over the cells of |grad Phi|  [V/m]
    field_max_cell: int
    field_max_centroid: Tuple[float, float]
    nodal_max: np.ndarray             # [ns + 1] max_v u_c(v), bitwise state values; [ns]: max_v (u_0 - u_e)(v)
    nodal_max_vertex: np.ndarray
    finite: bool                      # False: a value met on the way was not finite; the rest is unspecified
    net: np.ndarray                   # [nr, ns] the reactions' net gains (the model's)
    sign: np.ndarray                  # [ns] the species' charge numbers

    @property
    def source(self):
        """[ns] what the reactions and the field put in: sum_j net[j][s] reaction[j]; [0]: joule - collision_loss."""
        src = self.net.T.astype(np.float64) @ self.reaction
        src[0] = self.joule - self.collision_loss
        return src

    @property
    def imbalance(self):
        """[ns] rate_of_change - source + sum_t wall: the sum over all vertices of row c of the residual."""
        return self.rate_of_change - self.source + self.wall.sum(axis=0)

    @property
    def wall_current(self):
        """[n_tags] e sum_s sign_s wall[t][s] [A]: the conduction current into each boundary (ions plus the secondary
        electrons they release, minus the electrons that arrive)."""
        return elementary_charge * (self.wall[:, 1:] @ self.sign[1:])

    @property
    def power_joule(self):
        """e joule [W]."""
        return elementary_charge * self.joule

    @property
    def current(self):
        """e I_psi [A]."""
        return elementary_charge * self.induced_current

    @property
    def surface_charge(self):
        """eps0 q_g [C]: the charge on electrode g."""
        return epsilon_0 * self.group_sum

    @property
    def mean_energy_max(self):
        """the largest nodal mean energy exp(u_0 - u_e) [eV]."""
        return float(np.exp(self.nodal_max[-1]))


@dataclass
class Currents:
    """One call of :meth:`DeviceProblem.currents` (``fedm_currents``, include/fedm_hip.h has the formulae), in SI units:
    entry ``g`` belongs to weighting potential ``g``.  Axisymmetric: totals; planar: per metre of depth.  ``raw`` keeps
    the library's own sums (``conduction`` [1/s], ``displacement`` [V m/s], ``coupling`` [V m], ``induced_charge`` [1],
    ``capacitance`` [m])."""
    conduction: np.ndarray            # e sum_s Z_s int Gamma_s . (-grad psi_g)  [A; A/m planar]
    displacement: np.ndarray          # eps0 int grad(D_t Phi) . grad psi_g  [A; A/m planar]
    induced_charge: np.ndarray        # e sum_s Z_s int n_s psi_g  [C; C/m planar]
    coupling: np.ndarray              # int grad Phi . grad psi_g  [V m; V planar]
    capacitance: np.ndarray           # eps0 int grad psi_g . grad psi_h  [F; F/m planar]
    finite: bool                      # False: a value met on the way was not finite; the rest is unspecified
    raw: dict = field(default_factory=dict)

    @property
    def total(self):
        """conduction + displacement: the Shockley-Ramo current in the lead of each electrode."""
        return self.conduction + self.displacement


@dataclass
class CircuitState:
    """What the device holds of the external circuit (``fedm_circuit_get`` / ``fedm_circuit_advance``,
    include/fedm_hip.h has the scheme), in SI units: entry ``g`` belongs to electrode ``g``.  Axisymmetric: volts, amperes,
    siemens; planar: per metre of depth.  ``raw`` keeps the library's own ``conduction`` [1/s] and ``conductance``
    [1/(V s)]."""
    U: np.ndarray                     # the last advance's U^{n+1} (before the first: the initial potentials)  [V]
    U_old: np.ndarray                 # U^n
    U_old1: np.ndarray                # U^{n-1}
    dUdt: np.ndarray                  # the BDF2 quotient of the last advance  [V/s]
    lead_current: np.ndarray          # (V - U)/R of the last advance; an ideal source's linearised current  [A]
    conduction: np.ndarray            # e cond_g of the last measure  [A]
    conductance: np.ndarray           # e G_gh of the last measure  [S]
    flag: int                         # 0, or FEDM_CIRCUIT_* bits: U was left as it was
    raw: dict = field(default_factory=dict)

    @property
    def finite(self):
        return self.flag == 0


@dataclass
class FieldValues:
    """One call of :meth:`DeviceProblem.fields` (``fedm_fields``): ``nodal[k]`` the nodal values of request ``k`` in the
    caller's vertex order (None with ``nodal=False``), ``probes[k]`` its values at the probe points (None without
    ``probes=True``), ``finite`` False when a state value or a result was not finite, ``cg_iterations[k]`` the
    conjugate-gradient steps of a consistent projection (0 otherwise)."""
    names: list
    nodal: Optional[np.ndarray]
    probes: Optional[np.ndarray]
    finite: bool
    cg_iterations: np.ndarray

    def __getitem__(self, name):
        return self.nodal[self.names.index(name)]


def boundary_vertex_groups(cells, facet_tags, n_vertices, dirichlet_vertices, boundary_tags):
    """``int8 group[n_vertices]`` for :meth:`DeviceProblem.diagnostics_setup`: group ``g + 1`` holds the vertices of the
    facets tagged ``boundary_tags[g]`` (facet i lies opposite vertex i) that are in ``dirichlet_vertices``.  Host only.
    A vertex that would fall into two groups raises ``ValueError``."""
    boundary_tags = [int(t) for t in boundary_tags]
    if len(boundary_tags) > _lib.DIAG_MAX_GROUPS:
        raise ValueError(f"at most {_lib.DIAG_MAX_GROUPS} vertex groups, got {len(boundary_tags)}")
    group = np.zeros(int(n_vertices), dtype=np.int8)
    if not boundary_tags:
        return group
    if facet_tags is None:
        raise ValueError("vertex groups by boundary tag need the mesh's facet tags")
    cells = np.asarray(cells).reshape(-1, 3)
    tags = np.asarray(facet_tags).reshape(-1, 3)
    fixed = np.zeros(int(n_vertices), dtype=bool)
    fixed[np.asarray(dirichlet_vertices, dtype=np.int64)] = True
    for g, tag in enumerate(boundary_tags):
        member = np.zeros(int(n_vertices), dtype=bool)
        for i in range(3):
            hit = tags[:, i] == tag
            member[cells[hit, (i + 1) % 3]] = True
            member[cells[hit, (i + 2) % 3]] = True
        member &= fixed
        clash = np.nonzero(member & (group != 0))[0]
        if clash.size:
            raise ValueError(f"vertex {int(clash[0])} lies on boundary {tag} and on boundary "
                             f"{boundary_tags[int(group[clash[0]]) - 1]}: a vertex belongs to one group")
        group[member] = g + 1
    return group


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _part1by1(v):
    v = v.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    for shift, mask in ((16, 0x0000FFFF0000FFFF), (8, 0x00FF00FF00FF00FF),
                        (4, 0x0F0F0F0F0F0F0F0F), (2, 0x3333333333333333),
                        (1, 0x5555555555555555)):
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v


def z_curve_order(coords):
    """Vertex order along a Z-curve over the rank-quantised coordinates: on a tensor-product mesh,
    whatever its grading, 64 consecutive vertices form an 8x8 block."""
    ranks = []
    for d in range(2):
        _, inv = np.unique(coords[:, d], return_inverse=True)
        ranks.append(inv.astype(np.uint64))
    key = _part1by1(ranks[0]) | (_part1by1(ranks[1]) << np.uint64(1))
    return np.argsort(key, kind="stable")


def _vertex_spacing(coords, cells):
    """Mean |dx|, |dy| of the edges at every vertex: the metric in which a patch should be round."""
    cells = np.asarray(cells)
    n = coords.shape[0]
    e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]])
    d = np.abs(coords[e[:, 0]] - coords[e[:, 1]])
    ends = np.concatenate([e[:, 0], e[:, 1]])
    cnt = np.bincount(ends, minlength=n).astype(np.float64)
    acc = np.stack([np.bincount(ends, weights=np.concatenate([d[:, k], d[:, k]]), minlength=n) for k in (0, 1)], axis=1)
    h = acc / np.maximum(cnt, 1.0)[:, None]
    h[h <= 0.0] = h[h > 0.0].mean() if np.any(h > 0.0) else 1.0
    return h


def bisection_order(coords, spacing=None, leaf=64):
    """Vertex order by recursive median bisection (a k-d tree whose leaves are the 64-vertex
    slices): each split halves the vertex set across its longer side, measured in local mesh
    spacings, and puts a multiple of 64 vertices to the left, so that every slice is one leaf -- a
    compact patch on a locally refined unstructured mesh, where the quantised Z-curve tears patches
    apart.  Inside a leaf the bisection goes on down to single vertices (a Z-like local order)."""
    n = coords.shape[0]
    h = np.ones_like(coords) if spacing is None else spacing
    order = np.arange(n)
    stack = [(0, n)]
    while stack:
        a, b = stack.pop()
        m = b - a
        if m <= leaf:
            continue
        idx = order[a:b]
        p = coords[idx]
        ext = (p.max(axis=0) - p.min(axis=0)) / h[idx].mean(axis=0)
        d = 0 if ext[0] >= ext[1] else 1
        n_left = ((m + leaf - 1) // leaf + 1) // 2 * leaf
        order[a:b] = idx[np.argpartition(p[:, d], n_left - 1)]
        stack.append((a, a + n_left))
        stack.append((a + n_left, b))
    n_leaves = (n + leaf - 1) // leaf
    o = np.concatenate([order, np.full(n_leaves * leaf - n, -1, dtype=order.dtype)])
    g = leaf
    while g > 1:                                   # all leaves at once, one level per pass
        grp = o.reshape(-1, g)
        valid = grp >= 0
        safe = np.maximum(grp, 0)
        P, H = coords[safe], h[safe]
        lo = np.where(valid[..., None], P, np.inf).min(axis=1)
        hi = np.where(valid[..., None], P, -np.inf).max(axis=1)
        hm = np.where(valid[..., None], H, 0.0).sum(axis=1) / np.maximum(valid.sum(axis=1), 1)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            ext = (hi - lo) / hm
        d = np.where(np.nan_to_num(ext[:, 0], nan=0.0) >= np.nan_to_num(ext[:, 1], nan=0.0), 0, 1)
        key = np.where(valid, np.take_along_axis(P, d[:, None, None], axis=2)[..., 0], np.inf)
        o = np.take_along_axis(grp, np.argsort(key, axis=1, kind="stable"), axis=1).reshape(-1)
        g //= 2
    return o[o >= 0]


def cell_visits(order, cells, n_vertices, leaf=64):
    """Cell evaluations of the patch assembly under a vertex order: a cell is evaluated once by
    every slice that owns one of its vertices."""
    inv = np.empty(n_vertices, dtype=np.int64)
    inv[order] = np.arange(order.size)
    s = np.sort(inv[cells] // leaf, axis=1)
    return int(cells.shape[0] + (s[:, 1] != s[:, 0]).sum() + (s[:, 2] != s[:, 1]).sum())


def locality_order(coords, cells=None):
    """Internal vertex numbering of the device path (returns ``order``: new -> old).

    64 consecutive vertices are one slice = one assembly patch = one wavefront of matrix rows, so
    the order should make them compact: few halo vertices and redundant cell evaluations per patch,
    the neighbours of a matrix slice within a few cache lines, multigrid aggregates contiguous.
    Two candidates -- the Z-curve over rank-quantised coordinates (ideal on tensor-product meshes,
    whatever their grading) and recursive bisection in the metric of the local mesh spacing (for
    unstructured, locally refined meshes) -- and the one with fewer redundant cell evaluations is
    taken; without ``cells`` the Z-curve.  Deterministic: every rank computes the same order."""
    z = z_curve_order(coords)
    if cells is None or len(cells) == 0:
        return z
    cells = np.asarray(cells)
    kd = bisection_order(coords, _vertex_spacing(coords, cells))
    nv = coords.shape[0]
    return z if cell_visits(z, cells, nv) <= cell_visits(kd, cells, nv) else kd


def pattern_stats(coords, cells, reorder=True):
    """Host-side preprocessing alone (``fedm_pattern_stats``; runs without a GPU): slices, patch
    sizes and the LDS-accumulator clashes of the patch cell order, for the mesh as the device would
    number it."""
    lib = _lib.load()
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    order = locality_order(coords, cells) if reorder else np.arange(coords.shape[0])
    inv = np.empty(coords.shape[0], dtype=np.int64)
    inv[order] = np.arange(coords.shape[0])
    cdev = np.ascontiguousarray(coords[order])
    kdev = np.ascontiguousarray(inv[cells], dtype=np.int32)
    mesh = _lib.MeshDesc()
    mesh.n_vertices, mesh.n_cells = coords.shape[0], cells.shape[0]
    mesh.coords = _dp(cdev)
    mesh.cells = kdev.ctypes.data_as(C.POINTER(C.c_int32))
    out = (C.c_int64 * 12)()
    rc = lib.fedm_pattern_stats(C.byref(mesh), out)
    if rc != 0:
        raise RuntimeError(f"fedm_pattern_stats failed ({rc}): {_lib.last_error()}")
    keys = ("n_slices", "max_patch_cells", "max_patch_width", "max_patch_verts", "cell_visits",
            "owned_pairs", "bank_clashes", "nnz_blocks", "stored_blocks", "halo_vertices", "n_colours",
            "emission_blocks")
    return dict(zip(keys, (int(v) for v in out)))


def fieldsplit_tiles_stats(coords, cells, slices_per_tile=8, layers=3, reorder=True):
    """The tile tables of the species sweeps (csrc/fs_tiles.hip) built on the host alone
    (``fedm_fieldsplit_tiles_stats``; runs without a GPU), for the mesh as the device would number it, with the
    library's self-check of them (``violations`` must be 0)."""
    lib = _lib.load()
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    order = locality_order(coords, cells) if reorder else np.arange(coords.shape[0])
    inv = np.empty(coords.shape[0], dtype=np.int64)
    inv[order] = np.arange(coords.shape[0])
    cdev = np.ascontiguousarray(coords[order])
    kdev = np.ascontiguousarray(inv[cells], dtype=np.int32)
    mesh = _lib.MeshDesc()
    mesh.n_vertices, mesh.n_cells = coords.shape[0], cells.shape[0]
    mesh.coords = _dp(cdev)
    mesh.cells = kdev.ctypes.data_as(C.POINTER(C.c_int32))
    out = (C.c_int64 * 10)()
    rc = lib.fedm_fieldsplit_tiles_stats(C.byref(mesh), int(slices_per_tile), int(layers), out)
    if rc != 0:
        raise RuntimeError(f"fedm_fieldsplit_tiles_stats failed ({rc}): {_lib.last_error()}")
    keys = ("n_tiles", "row_width", "max_vertices", "max_rows", "total_rows", "total_vertices", "bytes", "violations",
            "lds_bytes_species_kernel", "lds_bytes_multigrid_kernel")
    return dict(zip(keys, (int(v) for v in out)))


# the counters of fedm_solver_path_stats, in its order (include/fedm_hip.h)
SOLVER_PATH_STATS = ("cycles", "steps_single", "steps_pair", "steps_last", "steps_dropped", "updates_made_up",
                     "second_passes", "fused_updates", "generic_updates", "deferred_norm", "nothing_to_solve",
                     "residual_only_right", "residual_only_wrong", "err_cache_served", "steps_used", "steps_ahead",
                     "steps_ahead_later", "solves", "breakdowns", "exhausted", "newton_max_it", "verified",
                     "verify_failed", "second_passes_device")

# fedm_pattern_info's / fedm_launched_assembly's numbering of the volume-assembly kernels
_VARIANTS = ("global colouring", "lds-patches/unrolled", "lds-patches", "lds-patches/one-pass",
             # the LMEA family's element kernels (fedm_launched_assembly only)
             "lmea/dual-number colours", "lmea/atomics", "lmea/element buffer, cell order",
             "lmea/element buffer, destination order", "lmea/element buffer, destination order, columns side by side")


class DeviceProblem:
    """Mesh + model + state resident on one MI355X."""

    def __init__(self, coords, cells, model: Model, facet_tags=None,
                 dirichlet_dofs=(), dirichlet_vals=(), device=0, reorder=True, n_owned=None,
                 identity_vertices=None, halo_depth=1):
        self.lib = _lib.load()
        self.model = model
        self.coords = np.ascontiguousarray(coords, dtype=np.float64)
        self.cells = np.ascontiguousarray(cells, dtype=np.int32)
        self.nv, self.nc = self.coords.shape[0], self.cells.shape[0]
        if self.coords.ndim != 2 or self.coords.shape[1] != 2 or self.cells.ndim != 2 or self.cells.shape[1] != 3:
            raise ValueError("DeviceProblem: coords must be (n_vertices, 2) and cells (n_cells, 3)")
        if self.nc and (self.cells.min() < 0 or self.cells.max() >= self.nv):
            raise ValueError("DeviceProblem: cell vertex index out of range")
        self.n_eq = model.n_eq
        self.n = self.nv * self.n_eq
        self._tags = None if facet_tags is None else np.ascontiguousarray(facet_tags, dtype=np.int8)
        # internal vertex numbering (the caller keeps seeing its own numbering)
        # multi-GPU: vertices [0, n_owned) are owned, the rest are ghosts (kept in place)
        self.n_owned = self.nv if n_owned is None else int(n_owned)
        self._order = np.arange(self.nv)
        if reorder:
            # (cells among the owned vertices: across GPUs the ghosts keep their place at the end)
            own_cells = self.cells[(self.cells < self.n_owned).all(axis=1)]
            self._order[:self.n_owned] = locality_order(self.coords[:self.n_owned], own_cells)
        self._inv = np.empty(self.nv, dtype=np.int64)
        self._inv[self._order] = np.arange(self.nv)
        neq = self.n_eq
        self._dof_new_of_old = (self._inv[:, None] * neq + np.arange(neq)[None, :]).ravel()
        ddofs = np.asarray(dirichlet_dofs, dtype=np.int64)
        self._ddofs = np.ascontiguousarray(self._dof_new_of_old[ddofs] if ddofs.size else ddofs,
                                           dtype=np.int32)
        self._dvals = np.ascontiguousarray(dirichlet_vals, dtype=np.float64)
        self._coords_dev = np.ascontiguousarray(self.coords[self._order])
        self._cells_dev = np.ascontiguousarray(self._inv[self.cells], dtype=np.int32)
        self._cell_order = None        # the caller's index of the device's cell k (None: the same)
        if isinstance(model, GdModel) and reorder and os.environ.get("FEDM_GD_CELL_ORDER", "1") != "0":
            # LMEA: the element kernels take 64 consecutive cells a workgroup and the gather kernel reads, for
            # consecutive matrix rows, the blocks of the cells around them -- cells in the order of their vertices
            # (nothing the caller passes or gets back is indexed by cell besides the facet tags)
            by_vertex = np.argsort(self._cells_dev.min(axis=1), kind="stable")
            self._cells_dev = np.ascontiguousarray(self._cells_dev[by_vertex])
            self._cell_order = by_vertex
            if self._tags is not None:
                self._tags = np.ascontiguousarray(self._tags.reshape(self.nc, 3)[by_vertex])
        tab = None
        if isinstance(model, GdModel):
            md = model.to_c()
        else:
            md, *tab = model.to_c_tabulated()
            if tab[0].size == 1:
                tab = None
        mesh = _lib.MeshDesc()
        mesh.n_vertices, mesh.n_cells = self.nv, self.nc
        mesh.coords = _dp(self._coords_dev)
        mesh.cells = self._cells_dev.ctypes.data_as(C.POINTER(C.c_int32))
        mesh.facet_tags = (self._tags.ctypes.data_as(C.POINTER(C.c_int8))
                           if self._tags is not None else None)
        mesh.n_dirichlet = self._ddofs.size
        mesh.dirichlet_dofs = self._ddofs.ctypes.data_as(C.POINTER(C.c_int32))
        mesh.dirichlet_vals = _dp(self._dvals)
        mesh.n_owned_vertices = self.n_owned
        # deep halos (partition.local_mesh(depth > 1)): the ghost vertices with identity rows (ghosts keep
        # their place in the internal numbering, so the caller's ids are the device's)
        self.halo_depth = int(halo_depth)
        if identity_vertices is not None and self.halo_depth > 1:
            self._identity = np.ascontiguousarray(identity_vertices, dtype=np.int32)
            if self._identity.size and (self._identity.min() < self.n_owned or self._identity.max() >= self.nv):
                raise ValueError("DeviceProblem: identity_vertices must be ghost vertices")
            mesh.n_identity_vertices = self._identity.size
            mesh.identity_vertices = self._identity.ctypes.data_as(C.POINTER(C.c_int32))
            mesh.halo_depth = self.halo_depth
        handle = C.c_void_p()
        wd = None if isinstance(model, GdModel) else model.walls_to_c()
        layers = None if isinstance(model, GdModel) else model.dielectric
        if layers is not None:  # dielectric layers (with or without walls and tables)
            tab_ptr, tab_x, tab_y = tab if tab is not None else (np.zeros(1, dtype=np.int32), np.zeros(0), np.zeros(0))
            dd = layers.to_c()
            rc = self.lib.fedm_ctx_create_dielectric(C.byref(mesh), C.byref(md), None if wd is None else C.byref(wd),
                                                     C.byref(dd), tab_ptr.size - 1,
                                                     tab_ptr.ctypes.data_as(C.POINTER(C.c_int32)), _dp(tab_x), _dp(tab_y),
                                                     int(device), C.byref(handle))
        elif wd is not None:    # 'flux source' walls (with or without tables)
            tab_ptr, tab_x, tab_y = tab if tab is not None else (np.zeros(1, dtype=np.int32), np.zeros(0), np.zeros(0))
            rc = self.lib.fedm_ctx_create_walls(C.byref(mesh), C.byref(md), C.byref(wd), tab_ptr.size - 1,
                                                tab_ptr.ctypes.data_as(C.POINTER(C.c_int32)), _dp(tab_x), _dp(tab_y),
                                                int(device), C.byref(handle))
        elif tab is not None:   # tabulated E/N coefficients: looked up in the element routines
            tab_ptr, tab_x, tab_y = tab
            rc = self.lib.fedm_ctx_create_tabulated(C.byref(mesh), C.byref(md), tab_ptr.size - 1,
                                                    tab_ptr.ctypes.data_as(C.POINTER(C.c_int32)), _dp(tab_x),
                                                    _dp(tab_y), int(device), C.byref(handle))
        else:
            create = self.lib.fedm_ctx_create_gd if isinstance(model, GdModel) else self.lib.fedm_ctx_create
            rc = create(C.byref(mesh), C.byref(md), int(device), C.byref(handle))
        if rc != 0:
            raise RuntimeError(f"fedm_ctx_create failed ({rc}): {_lib.last_error()}")
        self._h = handle
        # photoionisation: the Helmholtz operators and their hierarchies, once (host); the source is stale until the
        # first update, and again after everything that changes u_old
        self._photo_stale = False
        photo = None if isinstance(model, GdModel) else model.photoionization
        if photo is not None:
            from . import photo as photo_setup
            self.photo_levels = photo_setup.install(self.lib, self._h, photo, self._coords_dev, self._cells_dev,
                                                    self._tags, model.axisymmetric, model.quadrature_degree)
            self._photo_stale = True

    # -- lifetime ----------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.fedm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what} failed ({rc}): {_lib.last_error()}")
        if rc > 0:
            raise RuntimeError(f"{what}: {_lib.DIVERGED.get(rc, rc)}")

    # -- state --------------------------------------------------------------
    def _vec(self, a):
        """caller's dof order -> device order"""
        if a is None:
            return None
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        if a.size != self.n:
            raise ValueError(f"state vector must have {self.n} entries, got {a.size}")
        return np.ascontiguousarray(a.reshape(self.nv, self.n_eq)[self._order]).reshape(-1)

    def _back(self, a):
        """device order -> caller's dof order"""
        return np.ascontiguousarray(a.reshape(self.nv, self.n_eq)[self._inv]).reshape(-1)

    def set_state(self, u_new=None, u_old=None, u_old1=None):
        vs = [self._vec(v) for v in (u_new, u_old, u_old1)]
        self._check(self.lib.fedm_set_state(self._h, *[_dp(v) if v is not None else None for v in vs]),
                    "fedm_set_state")
        self._photo_stale = self._has_photo()

    def get_state(self):
        out = np.empty(self.n)
        self._check(self.lib.fedm_get_state(self._h, _dp(out)), "fedm_get_state")
        return self._back(out).reshape(self.nv, self.n_eq)

    def shift_state(self):
        self._check(self.lib.fedm_shift_state(self._h), "fedm_shift_state")
        self._photo_stale = self._has_photo()

    def reset_state(self):
        self._check(self.lib.fedm_reset_state(self._h), "fedm_reset_state")
        self._photo_stale = self._has_photo()

    def snapshot_state(self):
        """u, u_old, u_old1 into a device-side copy (fedm_state_snapshot)."""
        self._check(self.lib.fedm_state_snapshot(self._h), "fedm_state_snapshot")

    def restore_state(self):
        self._check(self.lib.fedm_state_restore(self._h), "fedm_state_restore")
        self._photo_stale = self._has_photo()

    def set_step(self, dt, dt_old):
        self._check(self.lib.fedm_set_step(self._h, float(dt), float(dt_old)), "fedm_set_step")

    def set_dirichlet_values(self, vals):
        v = np.ascontiguousarray(vals, dtype=np.float64)
        if v.size != self._ddofs.size:
            raise ValueError("wrong number of Dirichlet values")
        self._check(self.lib.fedm_set_dirichlet_values(self._h, _dp(v)), "fedm_set_dirichlet_values")

    def set_gd_fields(self, fields):
        """Nodal coefficient fields of the LMEA family, (n_fields, n_vertices) in the order
        of FEDM_GD_N_FIELDS (include/fedm_hip.h), caller's vertex numbering."""
        f = np.asarray(fields, dtype=np.float64)
        if f.shape != (self.model.n_fields, self.nv):
            raise ValueError(f"expected fields of shape {(self.model.n_fields, self.nv)}")
        f = np.ascontiguousarray(f[:, self._order])
        self._check(self.lib.fedm_gd_set_fields(self._h, _dp(f)), "fedm_gd_set_fields")

    def get_gd_fields(self):
        out = np.empty((self.model.n_fields, self.nv))
        self._check(self.lib.fedm_gd_get_fields(self._h, _dp(out)), "fedm_gd_get_fields")
        return np.ascontiguousarray(out[:, self._inv])

    def gd_prep_setup(self, tables, programs):
        """Install the on-device per-step refresh of the LMEA coefficient fields.
        ``tables``: list of (x, y) arrays; ``programs``: one dict per field row with keys
        kind ('keep' | 'table' | 'scaled_row' | 'me_old' | 'me' | 'ue_old') and, as needed,
        table, arg ('energy' | 'redfield'), scale, src_row."""
        import scipy.sparse as sp
        from . import amg
        x = self._coords_dev[self._cells_dev]
        d1, d2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
        det = np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
        vals = det[:, None, None] * ((np.ones((3, 3)) + np.eye(3)) / 24.0)[None]
        c = self._cells_dev.astype(np.int64)
        rows = np.broadcast_to(c[:, :, None], vals.shape).ravel()
        cols = np.broadcast_to(c[:, None, :], vals.shape).ravel()
        M = sp.coo_matrix((vals.ravel(), (rows, cols)), shape=(self.nv, self.nv)).tocsr()
        keep = []
        mass = amg._csr_struct(M, keep)
        ptr = np.zeros(len(tables) + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(t[0]) for t in tables])
        tx = np.ascontiguousarray(np.concatenate([np.asarray(t[0], float) for t in tables]) if tables else np.zeros(1))
        ty = np.ascontiguousarray(np.concatenate([np.asarray(t[1], float) for t in tables]) if tables else np.zeros(1))
        if len(programs) != self.model.n_fields:
            raise ValueError("one program per field row")
        progs = (_lib.GdFieldProg * len(programs))()
        for r, p in enumerate(programs):
            progs[r].kind = _lib.GDP[p["kind"]]
            progs[r].table = int(p.get("table", 0))
            progs[r].arg = _lib.GDP_ARG[p.get("arg", "energy")]
            progs[r].src_row = int(p.get("src_row", 0))
            progs[r].scale = float(p.get("scale", 1.0))
        self._check(self.lib.fedm_gd_prep_setup(self._h, C.byref(mass), len(tables),
                                                ptr.ctypes.data_as(C.POINTER(C.c_int32)), _dp(tx), _dp(ty),
                                                progs), "fedm_gd_prep_setup")

    def gd_prep_step(self):
        self._check(self.lib.fedm_gd_prep_step(self._h), "fedm_gd_prep_step")

    def get_gd_reduced_field(self):
        """The projected reduced electric field of the last :meth:`gd_prep_step` (what its E/N look-ups were
        evaluated at), caller's vertex numbering (``fedm_debug_gd_reduced_field``)."""
        out = np.empty(self.nv)
        self._check(self.lib.fedm_debug_gd_reduced_field(self._h, _dp(out)), "fedm_debug_gd_reduced_field")
        return np.ascontiguousarray(out[self._inv])

    def gd_update_mean_energy(self):
        self._check(self.lib.fedm_gd_update_mean_energy(self._h), "fedm_gd_update_mean_energy")

    def get_state_old(self):
        out = np.empty(self.n)
        self._check(self.lib.fedm_get_state_old(self._h, _dp(out)), "fedm_get_state_old")
        return self._back(out).reshape(self.nv, self.n_eq)

    def set_ext_source_program(self, species, ops, consts, n_params):
        """Expression source evaluated on the device: the postfix program of
        :func:`fedm_amd.forms.expression_program` (``fedm_ext_source_program``)."""
        ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 2)
        consts = np.ascontiguousarray(consts, dtype=np.float64)
        self._check(self.lib.fedm_ext_source_program(
            self._h, int(species), int(ops.shape[0]), ops.ctypes.data_as(C.POINTER(C.c_int32)),
            int(consts.size), _dp(consts if consts.size else np.zeros(1)), int(n_params)), "fedm_ext_source_program")

    def eval_ext_source(self, species, params):
        """Fill the species' source table with the program's values for these parameter values."""
        p = np.ascontiguousarray(params if len(params) else [0.0], dtype=np.float64)
        self._check(self.lib.fedm_ext_source_eval(self._h, int(species), _dp(p)), "fedm_ext_source_eval")

    def set_ext_source(self, species, nodal):
        v = np.ascontiguousarray(nodal, dtype=np.float64)
        self._check(self.lib.fedm_set_ext_source(self._h, int(species), _dp(v)), "fedm_set_ext_source")

    def get_ext_source(self, species):
        """The species' source table as it stands on the device, (n_cells, nodes) (``fedm_debug_get_ext_source``)."""
        degrees = (self.model.source_table_degrees() if hasattr(self.model, "source_table_degrees")
                   else list(getattr(self.model, "ext_source_degree", ())))
        k = degrees[int(species)] if 0 <= int(species) < len(degrees) else 0
        out = np.empty((self.nc, (k + 1) * (k + 2) // 2))          # (no source: the library refuses, nothing is written)
        self._check(self.lib.fedm_debug_get_ext_source(self._h, int(species), _dp(out)), "fedm_debug_get_ext_source")
        return out

    # -- photoionisation (Helmholtz sources, csrc/photo.hip) ---------------------------
    def _has_photo(self):
        return getattr(self.model, "photoionization", None) is not None

    def photo_update(self):
        """The photoionisation source of the state as it stands (``fedm_photo_update``): the ionisation rate at
        ``u_old``, one warm-started CG solve per Helmholtz term, the targets' source tables.  Explicit lag: it is
        frozen until ``u_old`` changes (``shift_state``, ``set_state``, ``reset_state``, ``restore_state`` mark it
        stale; :meth:`newton_solve` updates a stale source first), so a step retried with a smaller ``dt`` reuses it.
        Returns the CG iterations per term, kept in ``last_photo_iterations`` too."""
        if not self._has_photo():
            raise RuntimeError("the model has no photoionisation source")
        ph = self.model.photoionization
        its = (C.c_int * _lib.PHOTO_MAX_TERMS)()
        rc = self.lib.fedm_photo_update(self._h, float(ph.rtol), int(ph.max_it), its)
        self.last_photo_iterations = [int(v) for v in its[:len(ph.c)]]
        if rc == 3:
            raise RuntimeError(f"fedm_photo_update: conjugate gradients stopped at max_it = {ph.max_it} "
                               f"(iterations per term {self.last_photo_iterations})")
        self._check(rc, "fedm_photo_update")
        self._photo_stale = False
        return self.last_photo_iterations

    def get_photo(self):
        """``(y, g)`` of the last update: the Helmholtz solutions ``y[n_terms, n_vertices]`` and the load vector
        ``g[n_vertices]``, caller's vertex numbering (``fedm_photo_get``)."""
        n_terms = len(self.model.photoionization.c) if self._has_photo() else 1
        y, g = np.empty((n_terms, self.nv)), np.empty(self.nv)
        self._check(self.lib.fedm_photo_get(self._h, _dp(y), _dp(g)), "fedm_photo_get")
        return np.ascontiguousarray(y[:, self._inv]), np.ascontiguousarray(g[self._inv])

    PHOTO_STATS = ("updates", "cg_iterations_0", "cg_iterations_1", "cg_iterations_2", "cg_iterations_3", "vcycles",
                   "exhausted", "reserved")

    def photo_stats(self, reset=False):
        """Counters of the photoionisation updates since the set-up or the last reset (``fedm_photo_stats``)."""
        out = (C.c_int64 * 8)()
        self._check(self.lib.fedm_photo_stats(self._h, out, 1 if reset else 0), "fedm_photo_stats")
        return dict(zip(self.PHOTO_STATS, (int(v) for v in out)))

    # -- discharge diagnostics (csrc/diag.hip) ------------------------------------------
    def dirichlet_vertices(self, component=None):
        """The caller's vertices with a Dirichlet row of ``component`` (default: the last one, the potential)."""
        comp = self.n_eq - 1 if component is None else int(component)
        d = self._ddofs.astype(np.int64)
        return np.unique(self._order[d[d % self.n_eq == comp] // self.n_eq])

    def diagnostics_setup(self, weighting_potential=None, vertex_groups=None, n_groups=None):
        """What :meth:`diagnostics` needs once (``fedm_diag_setup``), both in the caller's numbering:
        ``weighting_potential``: nodal P1 psi ``[n_vertices]`` of the induced current (None: no current);
        ``vertex_groups``: ``int8 [n_vertices]``, 0 or the group 1..8 whose Poisson rows are summed
        (:func:`boundary_vertex_groups`; None: no groups); ``n_groups``: how many sums come back (default: the largest
        group present).  Replaces an earlier set-up."""
        if isinstance(self.model, GdModel):
            raise RuntimeError("diagnostics: LFA models only (the LMEA family is not covered)")
        psi = grp = None
        n_groups = int(n_groups or 0)
        if weighting_potential is not None:
            psi = np.asarray(weighting_potential, dtype=np.float64).reshape(-1)
            if psi.size != self.nv:
                raise ValueError(f"weighting_potential must have {self.nv} entries, got {psi.size}")
            psi = np.ascontiguousarray(psi[self._order])
        if vertex_groups is not None:
            grp = np.asarray(vertex_groups).reshape(-1)
            if grp.size != self.nv:
                raise ValueError(f"vertex_groups must have {self.nv} entries, got {grp.size}")
            if grp.size and (grp.min() < 0 or grp.max() > _lib.DIAG_MAX_GROUPS):
                raise ValueError(f"vertex_groups holds 0 or a group 1..{_lib.DIAG_MAX_GROUPS}")
            n_groups = max(int(grp.max()) if grp.size else 0, n_groups)
            if n_groups > _lib.DIAG_MAX_GROUPS:
                raise ValueError(f"at most {_lib.DIAG_MAX_GROUPS} vertex groups")
            grp = np.ascontiguousarray(grp[self._order], dtype=np.int8) if n_groups else None
        else:
            n_groups = 0
        self._check(self.lib.fedm_diag_setup(self._h, _dp(psi) if psi is not None else None,
                                             grp.ctypes.data_as(C.POINTER(C.c_int8)) if grp is not None else None,
                                             n_groups), "fedm_diag_setup")
        self._diag_groups = n_groups

    def diagnostics(self, window=None, state="new"):
        """The discharge's observables from the resident state (``fedm_diagnostics``): one pass over the cells, one
        over the vertices, a read-back of a few hundred bytes.  ``window``: ``(r_lo, r_hi, z_lo, z_hi)`` of the second
        field maximum (None: the whole mesh); ``state``: "new" or "old".  Returns a :class:`Diagnostics`."""
        if isinstance(self.model, GdModel):
            raise RuntimeError("diagnostics: LFA models only (the LMEA family is not covered)")
        if state not in ("new", "old"):
            raise ValueError('diagnostics: state is "new" or "old"')
        opts = _lib.DiagOpts()
        opts.state = 0 if state == "new" else 1
        opts.r_lo, opts.r_hi, opts.z_lo, opts.z_hi = ((-np.inf, np.inf, -np.inf, np.inf) if window is None
                                                      else [float(w) for w in window])
        out = _lib.DiagOut()
        self._check(self.lib.fedm_diagnostics(self._h, C.byref(opts), C.byref(out)), "fedm_diagnostics")
        ns = self.model.n_species
        vert = np.array(out.nodal_max_vertex[:ns], dtype=np.int64)
        return Diagnostics(
            species_integral=np.array(out.species_integral[:ns]),
            group_sum=np.array(out.group_sum[:getattr(self, "_diag_groups", 0)]),
            induced_current=float(out.induced_current),
            field_max=float(out.field_max), field_max_cell=int(out.field_max_cell),
            field_max_centroid=tuple(out.field_max_centroid),
            window_max=float(out.window_max), window_max_cell=int(out.window_max_cell),
            window_max_centroid=tuple(out.window_max_centroid),
            nodal_max=np.array(out.nodal_max[:ns]),
            nodal_max_vertex=np.where(vert >= 0, self._order[np.maximum(vert, 0)], -1),
            finite=bool(out.finite), Z=np.asarray(self.model.Z, dtype=np.float64)[:ns],
            linear_representation=not self.model.log_representation)

    # -- particle and energy balance of LMEA models (csrc/gd_balance.hip) ------------------
    def facet_tags(self):
        """The boundary tags ``[n_cells, 3]`` in the caller's cell order (None without tags)."""
        if self._tags is None:
            return None
        tags = self._tags.reshape(self.nc, 3)
        if self._cell_order is None:
            return tags
        out = np.empty_like(tags)
        out[self._cell_order] = tags
        return out

    def balance_setup(self, weighting_potential=None, vertex_groups=None, n_groups=None):
        """What :meth:`balance` may use (``fedm_gd_balance_setup``), both in the caller's numbering:
        ``weighting_potential``: nodal P1 psi ``[n_vertices]`` of the induced current (None: no current);
        ``vertex_groups``: ``int8 [n_vertices]``, 0 or the group 1..8 whose Poisson rows are summed
        (:func:`boundary_vertex_groups`; None: no groups); ``n_groups``: how many sums come back (default: the largest
        group present).  Replaces an earlier set-up."""
        if not isinstance(self.model, GdModel):
            raise RuntimeError("balance: LMEA models only (diagnostics() has the LFA family's observables)")
        psi = grp = None
        n_groups = int(n_groups or 0)
        if weighting_potential is not None:
            psi = np.asarray(weighting_potential, dtype=np.float64).reshape(-1)
            if psi.size != self.nv:
                raise ValueError(f"weighting_potential must have {self.nv} entries, got {psi.size}")
            psi = np.ascontiguousarray(psi[self._order])
        if vertex_groups is not None:
            grp = np.asarray(vertex_groups).reshape(-1)
            if grp.size != self.nv:
                raise ValueError(f"vertex_groups must have {self.nv} entries, got {grp.size}")
            if grp.size and (grp.min() < 0 or grp.max() > _lib.GD_BAL_MAX_GROUPS):
                raise ValueError(f"vertex_groups holds 0 or a group 1..{_lib.GD_BAL_MAX_GROUPS}")
            n_groups = max(int(grp.max()) if grp.size else 0, n_groups)
            grp = np.ascontiguousarray(grp[self._order], dtype=np.int8) if n_groups else None
        else:
            n_groups = 0
        self._check(self.lib.fedm_gd_balance_setup(self._h, _dp(psi) if psi is not None else None,
                                                   grp.ctypes.data_as(C.POINTER(C.c_int8)) if grp is not None else None,
                                                   n_groups), "fedm_gd_balance_setup")
        self._balance_groups = n_groups

    def balance(self):
        """The particle and energy balance at the state the residual of the current step sees (``fedm_gd_balance``): a
        pass over the cells, one over the tagged facets, one over the vertices, a read-back of 880 bytes.  Returns a
        :class:`Balance`."""
        if not isinstance(self.model, GdModel):
            raise RuntimeError("balance: LMEA models only (diagnostics() has the LFA family's observables)")
        out = _lib.GdBalanceOut()
        self._check(self.lib.fedm_gd_balance(self._h, C.byref(out)), "fedm_gd_balance")
        ns, nr, nt = self.model.n_species, self.model.n_reactions, len(self.model.ref)
        vert = np.array(out.nodal_max_vertex[:ns + 1], dtype=np.int64)
        cell = int(out.field_max_cell)
        if cell >= 0 and self._cell_order is not None:
            cell = int(self._cell_order[cell])
        return Balance(
            content=np.array(out.content[:ns]), rate_of_change=np.array(out.rate_of_change[:ns]),
            reaction=np.array(out.reaction[:nr]), collision_loss=float(out.collision_loss), joule=float(out.joule),
            wall=np.array([list(out.wall[t][:ns]) for t in range(nt)]).reshape(nt, ns),
            ion_flux=np.array(out.ion_flux[:nt]), induced_current=float(out.induced_current),
            group_sum=np.array(out.group_sum[:getattr(self, "_balance_groups", 0)]),
            field_max=float(out.field_max), field_max_cell=cell, field_max_centroid=tuple(out.field_max_centroid),
            nodal_max=np.array(out.nodal_max[:ns + 1]),
            nodal_max_vertex=np.where(vert >= 0, self._order[np.maximum(vert, 0)], -1),
            finite=bool(out.finite), net=np.asarray(self.model.net, dtype=np.int64).reshape(nr, -1)[:, :ns],
            sign=np.asarray(self.model.sign, dtype=np.float64)[:ns])

    # -- electrode currents (csrc/currents.hip) --------------------------------------------
    def currents_setup(self, potentials=None, boundary_tags=None, rtol=1e-10, max_it=2000, multigrid=True,
                       max_coarse=600, nu=1, omega=0.67, theta=0.08):
        """What :meth:`currents` needs once.  Either ``potentials``: nodal P1 weighting potentials
        ``[n_psi, n_vertices]`` in the caller's numbering, taken as they are (``fedm_currents_setup``); or
        ``boundary_tags``: electrode ``g`` is the potential-Dirichlet vertices of the facets tagged
        ``boundary_tags[g]`` (:func:`boundary_vertex_groups`; a vertex in two groups raises ``ValueError``), and
        ``psi_g`` -- 1 on it, 0 on every other Dirichlet vertex of the potential, natural conditions elsewhere -- is
        solved for on the device (``fedm_currents_solve``): the host assembles ``K_w`` in the device's numbering once
        (``photo.helmholtz_matrices``), eliminates the Dirichlet vertices, builds the hierarchy (``amg.build_hierarchy``;
        Jacobi alone with ``multigrid=False`` or below ``max_coarse`` vertices) and the right-hand sides
        ``-K_w psi_D``; ``rtol``, ``max_it``: of the conjugate gradients, ``|r| <= rtol |b|``.  At most 8 potentials.
        Replaces an earlier set-up.  Returns the CG iterations per potential (empty without a solve), kept in
        ``last_currents_iterations`` too."""
        if (potentials is None) == (boundary_tags is None):
            raise ValueError("currents_setup: give either potentials or boundary_tags")
        # (the count and the iterations follow the library: a refused set-up leaves the earlier one in place, here too)
        if potentials is not None:
            psi = np.atleast_2d(np.asarray(potentials, dtype=np.float64))
            if psi.ndim != 2 or psi.shape[1] != self.nv:
                raise ValueError(f"potentials must be [n_psi, {self.nv}], got {psi.shape}")
            if not 1 <= psi.shape[0] <= _lib.CURRENTS_MAX:
                raise ValueError(f"1 to {_lib.CURRENTS_MAX} weighting potentials, got {psi.shape[0]}")
            psi = np.ascontiguousarray(psi[:, self._order])
            self._check(self.lib.fedm_currents_setup(self._h, psi.shape[0], _dp(psi)), "fedm_currents_setup")
            self._currents_n, self.last_currents_iterations = psi.shape[0], []
            return []
        from . import amg, photo
        tags = [int(t) for t in boundary_tags]
        if not 1 <= len(tags) <= _lib.CURRENTS_MAX:
            raise ValueError(f"1 to {_lib.CURRENTS_MAX} electrodes, got {len(tags)}")
        if not getattr(self.model, "poisson", True):
            raise RuntimeError("currents_setup: the model has no Poisson equation")
        fixed_caller = self.dirichlet_vertices()
        group = boundary_vertex_groups(self.cells, self.facet_tags(), self.nv, fixed_caller, tags)
        fixed = np.zeros(self.nv, dtype=bool)
        fixed[self._inv[fixed_caller]] = True                       # the device's numbering from here on
        group_dev = group[self._order]
        psi = np.zeros((len(tags), self.nv))
        for g in range(len(tags)):
            psi[g, group_dev == g + 1] = 1.0
        K, _ = photo.helmholtz_matrices(self._coords_dev, self._cells_dev.astype(np.int64), self.model.axisymmetric,
                                        self.model.quadrature_degree)
        A = photo.eliminate(K, fixed)
        rhs = -(K @ psi.T).T
        rhs[:, fixed] = 0.0
        rhs = np.ascontiguousarray(rhs)
        levels = [(A, None)]
        if multigrid:
            levels = amg.build_hierarchy(A, theta=theta, max_coarse=max_coarse, fixed=fixed, coords=self._coords_dev)
        self._check(self.lib.fedm_currents_setup(self._h, len(tags), _dp(psi)), "fedm_currents_setup")
        self._currents_n = len(tags)
        self.currents_levels = [a.shape[0] for a, _ in levels]
        # (what was solved, in the device's numbering: the hierarchy, the right-hand sides, the conductors' vertices)
        self.currents_system = (levels, rhs, fixed)
        return self.currents_solve(levels, rhs, rtol, max_it, nu=nu, omega=omega)

    def currents_solve(self, levels, rhs, rtol=1e-10, max_it=2000, nu=1, omega=0.67):
        """``fedm_currents_solve`` with a hierarchy ``[(A_l, P_l)]`` of :func:`fedm_amd.amg.build_hierarchy` (one level:
        Jacobi) and right-hand sides ``[n_psi, n_vertices]``, both in the DEVICE's numbering.  A solve that stops at
        ``max_it`` or meets a NaN raises ``RuntimeError`` and leaves the installed potentials as they were."""
        from . import amg
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        h, held = amg.pack_hierarchy(levels, nu, omega)
        its = (C.c_int * _lib.CURRENTS_MAX)()
        rc = self.lib.fedm_currents_solve(self._h, C.byref(h), _dp(rhs), float(rtol), int(max_it), its)
        self.last_currents_iterations = [int(v) for v in its[:getattr(self, "_currents_n", 0)]]
        if rc == 3:
            raise RuntimeError(f"fedm_currents_solve: conjugate gradients stopped at max_it = {max_it} "
                               f"(iterations per potential {self.last_currents_iterations})")
        if rc == 2:
            raise RuntimeError("fedm_currents_solve: NaN or an operator that is not positive definite")
        self._check(rc, "fedm_currents_solve")
        return self.last_currents_iterations

    def currents_psi(self):
        """The installed weighting potentials ``[n_psi, n_vertices]`` in the caller's numbering
        (``fedm_currents_get_psi``)."""
        out = np.empty((_lib.CURRENTS_MAX, self.nv))        # (room for whatever the library holds)
        self._check(self.lib.fedm_currents_get_psi(self._h, _dp(out)), "fedm_currents_get_psi")
        return np.ascontiguousarray(out[:getattr(self, "_currents_n", 0), self._inv])

    def currents(self):
        """The electrode currents of the resident state (``fedm_currents``): one pass over the cells, a one-workgroup
        finish, a read-back of under a kilobyte.  LFA: the fluxes at ``u_new``; LMEA: the fluxes the residual of the
        current step sees.  Returns a :class:`Currents`."""
        out = _lib.CurrentsOut()
        self._check(self.lib.fedm_currents(self._h, C.byref(out)), "fedm_currents")
        n = int(out.n_psi)
        raw = dict(conduction=np.array(out.conduction[:n]), displacement=np.array(out.displacement[:n]),
                   coupling=np.array(out.coupling[:n]), induced_charge=np.array(out.induced_charge[:n]),
                   capacitance=np.array([list(out.capacitance[g][:n]) for g in range(n)]).reshape(n, n))
        return Currents(conduction=elementary_charge * raw["conduction"], displacement=epsilon_0 * raw["displacement"],
                        induced_charge=elementary_charge * raw["induced_charge"], coupling=raw["coupling"].copy(),
                        capacitance=epsilon_0 * raw["capacitance"], finite=bool(out.finite), raw=raw)

    # -- dielectric layers (csrc/dielectric.hip) ------------------------------------------
    def set_layer_voltage(self, voltages):
        """The voltage of the conductor behind every layer, ``{tag: U}`` (tags as the mesh numbers them; a layer that
        is not named keeps its voltage), from the next assembly on (``fedm_dielectric_set_voltage``)."""
        layers = getattr(self.model, "dielectric", None)
        if layers is None:
            raise ValueError("set_layer_voltage: this problem has no dielectric layer")
        if not hasattr(self, "_layer_voltage"):      # what the context was created with, then what was set here
            self._layer_voltage = {t: float(layers.voltage.get(t, 0.0)) for t in layers.tags()}
        new = dict(self._layer_voltage)
        for t, u in dict(voltages).items():
            if int(t) not in new:
                raise ValueError(f"set_layer_voltage: tag {t} is no dielectric layer of this problem")
            new[int(t)] = float(u)
        U = (C.c_double * _lib.MAX_TAGS)()
        for t, u in new.items():
            U[t - 1] = u
        self._check(self.lib.fedm_dielectric_set_voltage(self._h, U), "fedm_dielectric_set_voltage")
        self._layer_voltage = new

    def dielectric_accept(self):
        """After an accepted step (and its state shift): the surface charge of the accepted state becomes q^n, the
        one before it q^(n-1) (``fedm_dielectric_accept``; no read-back)."""
        self._check(self.lib.fedm_dielectric_accept(self._h), "fedm_dielectric_accept")
        self._layers_solved = False

    def accept_layers(self):
        """What the time loops call after their state shift: :meth:`dielectric_accept` if the model has layers and a
        Newton solve has succeeded since the last accept (the first shift of a run comes before any solve)."""
        if getattr(self.model, "dielectric", None) is not None and getattr(self, "_layers_solved", False):
            self.dielectric_accept()

    def dielectric_charge(self, vertices=True):
        """Per layer tag the surface charge ``sum_a q_a`` and the layer's displacement charge ``eps0 eps_r/d int (Phi -
        U) 2 pi r ds`` [C; C/m planar] and its voltage; with ``vertices`` also ``q`` and ``q_old`` per vertex in the
        caller's numbering, 0 off the layers (``fedm_dielectric_get``)."""
        tot = _lib.DielectricTotals()
        q, qo = (np.zeros(self.nv), np.zeros(self.nv)) if vertices else (None, None)
        self._check(self.lib.fedm_dielectric_get(self._h, C.byref(tot), None if q is None else _dp(q),
                                                 None if qo is None else _dp(qo)), "fedm_dielectric_get")
        tags = self.model.dielectric.tags() if getattr(self.model, "dielectric", None) is not None else []
        out = dict(charge={t: tot.charge[t - 1] for t in tags}, displacement={t: tot.displacement[t - 1] for t in tags},
                   voltage={t: tot.voltage[t - 1] for t in tags}, n_layer_vertices=int(tot.n_layer_vertices))
        if vertices:
            out["q"], out["q_old"] = q[self._inv], qo[self._inv]
        return out

    def set_dielectric_charge(self, q=None, q_old=None):
        """``q^n`` and ``q^(n-1)`` per vertex (caller's numbering; entries off the layers are ignored), for restarts
        (``fedm_dielectric_set``).  A solved step that was still waiting for its accept is dropped with the history
        it belonged to."""
        self._layers_solved = False
        dev = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(self.nv)[self._order])
               for a in (q, q_old)]
        self._check(self.lib.fedm_dielectric_set(self._h, *[None if a is None else _dp(a) for a in dev]),
                    "fedm_dielectric_set")

    # -- external circuit (csrc/circuit.hip) ----------------------------------------------
    def circuit_setup(self, resistance, capacitance=0.0, initial=0.0, electrode_of_entry=None, boundary_tags=None):
        """What :meth:`circuit_measure` and :meth:`circuit_advance` need once (``fedm_circuit_setup``), after
        :meth:`currents_setup`: per electrode of that set-up a series ``resistance`` [ohm] (0: an ideal source), a stray
        ``capacitance`` to ground [F] and the ``initial`` potential [V] -- scalars or one value each.  The Dirichlet
        entries that get an electrode's potential: ``electrode_of_entry``, ``int8`` per entry of ``dirichlet_dofs`` in
        the order :meth:`set_dirichlet_values` takes (-1: left alone); or ``boundary_tags``: electrode ``g`` is the
        potential's Dirichlet entries on the vertices of the facets tagged ``boundary_tags[g]``
        (:func:`boundary_vertex_groups`, as :meth:`currents_setup` groups them).  Replaces an earlier set-up."""
        n = int(getattr(self, "_currents_n", 0))
        if n == 0:
            raise RuntimeError("circuit_setup: currents_setup has not been called")
        if (electrode_of_entry is None) == (boundary_tags is None):
            raise ValueError("circuit_setup: give either electrode_of_entry or boundary_tags")
        d = _lib.CircuitDesc()
        for name, val in (("R", resistance), ("Cp", capacitance), ("U0", initial)):
            v = np.broadcast_to(np.asarray(val, dtype=np.float64), (n,)) if np.ndim(val) == 0 else np.asarray(val, dtype=np.float64)
            if v.shape != (n,):
                raise ValueError(f"circuit_setup: {n} electrodes, got {v.shape} values")
            for g in range(n):
                getattr(d, name)[g] = float(v[g])
        if boundary_tags is not None:
            tags = [int(t) for t in boundary_tags]
            if len(tags) != n:
                raise ValueError(f"circuit_setup: {n} electrodes, got {len(tags)} boundary tags")
            group = boundary_vertex_groups(self.cells, self.facet_tags(), self.nv, self.dirichlet_vertices(), tags)
            dd = self._ddofs.astype(np.int64)
            entry = np.where(dd % self.n_eq == self.n_eq - 1, group[self._order[dd // self.n_eq]].astype(np.int64) - 1, -1)
        else:
            entry = np.asarray(electrode_of_entry).reshape(-1)
            if entry.size != self._ddofs.size:
                raise ValueError(f"circuit_setup: {self._ddofs.size} Dirichlet entries, got {entry.size}")
        entry = np.ascontiguousarray(entry, dtype=np.int8)
        d.n = n
        d.electrode_of_entry = entry.ctypes.data_as(C.POINTER(C.c_int8))
        self._check(self.lib.fedm_circuit_setup(self._h, C.byref(d)), "fedm_circuit_setup")
        self.circuit_entries = entry

    def circuit_measure(self):
        """After an accepted step (and once before the first): the history of the electrodes' potentials moves on and the
        conduction and the conductance of ``u_new`` are formed, all on the device (``fedm_circuit_measure``)."""
        self._check(self.lib.fedm_circuit_measure(self._h), "fedm_circuit_measure")

    def _circuit_state(self, out):
        n = int(out.n)
        raw = dict(conduction=np.array(out.conduction[:n]),
                   conductance=np.array([list(out.conductance[g][:n]) for g in range(n)]).reshape(n, n))
        return CircuitState(U=np.array(out.U[:n]), U_old=np.array(out.U_old[:n]), U_old1=np.array(out.U_old1[:n]),
                            dUdt=np.array(out.dUdt[:n]), lead_current=np.array(out.lead_current[:n]),
                            conduction=elementary_charge * raw["conduction"],
                            conductance=elementary_charge * raw["conductance"], flag=int(out.flag), raw=raw)

    def circuit_advance(self, voltages, read=False):
        """The electrodes' potentials at the end of the step ``set_step`` has set, for the sources' ``voltages`` there,
        written into the Dirichlet values the next solve reads (``fedm_circuit_advance``).  ``read``: read the record
        back (a :class:`CircuitState`; the call's only synchronisation); otherwise None."""
        V = np.zeros(_lib.CURRENTS_MAX)
        v = np.asarray(voltages, dtype=np.float64).reshape(-1)
        if v.size != getattr(self, "_currents_n", 0):
            raise ValueError(f"circuit_advance: {getattr(self, '_currents_n', 0)} electrodes, got {v.size} voltages")
        V[:v.size] = v
        out = _lib.CircuitState() if read else None
        self._check(self.lib.fedm_circuit_advance(self._h, _dp(V), C.byref(out) if read else None), "fedm_circuit_advance")
        return self._circuit_state(out) if read else None

    def circuit_get(self):
        """What the device holds of the circuit (``fedm_circuit_get``): a :class:`CircuitState`."""
        out = _lib.CircuitState()
        self._check(self.lib.fedm_circuit_get(self._h, C.byref(out)), "fedm_circuit_get")
        return self._circuit_state(out)

    # -- field output (csrc/fields.hip) ---------------------------------------------------
    def fields_setup(self, consistent=False):
        """What :meth:`fields` needs once (``fedm_fields_setup``): the vertex lists, the lumped mass and the results'
        buffers on the device; ``consistent``: the P1 mass matrix of the plain measure as well, assembled here once (the
        way ``photo.install`` assembles its operators), for ``projection="consistent"``.  Replaces an earlier set-up and
        drops its probe points."""
        if isinstance(self.model, GdModel):
            raise RuntimeError("fields: LFA models only (the LMEA family is not covered)")
        mass = None
        if consistent:
            from . import amg, field_output
            keep = []
            mass = amg._csr_struct(field_output.mass_matrix(self._coords_dev, self._cells_dev), keep)
        self._check(self.lib.fedm_fields_setup(self._h, C.byref(mass) if mass is not None else None), "fedm_fields_setup")
        self._fields_ready, self._n_probe_points = True, 0

    def probe_setup(self, points):
        """Probe points ``[n, 2]`` for :meth:`fields` (``fedm_probe_setup``): the cell that contains each point and its
        barycentric weights there are found here (``field_output.locate_points``: ties on an edge or a vertex go to the
        lowest cell index; a point outside the mesh is a ``ValueError`` naming it).  Returns ``(cells, weights)``."""
        from . import field_output
        if not getattr(self, "_fields_ready", False):
            self.fields_setup()
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        cell, w = field_output.locate_points(self.coords, self.cells, pts)
        verts = np.ascontiguousarray(self._inv[self.cells[cell]], dtype=np.int32)
        w = np.ascontiguousarray(w)
        self._check(self.lib.fedm_probe_setup(self._h, int(pts.shape[0]), verts.ctypes.data_as(C.POINTER(C.c_int32)),
                                              _dp(w)), "fedm_probe_setup")
        self._n_probe_points = int(pts.shape[0])
        return cell, w

    def fields(self, requests, t_out=None, t_old=None, t=None, projection="lumped", rtol=1e-10, nodal=True,
               probes=False, max_it=10000, species_names=None):
        """Derived fields of the resident state (``fedm_fields``; include/fedm_hip.h has the definitions).
        ``requests``: up to 8 names (``"E_norm"``, ``"E_r"``, ``"E_z"``, ``"charge"``, ``"state:e"``, ``"density:s"``,
        ``"rate:j"``, ``"flux_r:s"``, ``"flux_z:s"``) or ``(kind, index)`` pairs.  With ``t_out``, ``t_old`` and ``t``
        the result is ``X(u_old) + (t_out - t_old) (X(u_new) - X(u_old)) / (t - t_old)``, ``file_output``'s blend;
        without them ``X(u_new)``.  ``projection``: "lumped" or "consistent" (after ``fields_setup(consistent=True)``;
        conjugate gradients to ``rtol``).  Returns a :class:`FieldValues`: ``nodal [n_req, n_vertices]`` in the caller's
        vertex order (ghost entries 0) unless ``nodal=False``, ``probes [n_req, n_points]`` with ``probes=True``."""
        from . import field_output
        if isinstance(self.model, GdModel):
            raise RuntimeError("fields: LFA models only (the LMEA family is not covered)")
        if not getattr(self, "_fields_ready", False):
            self.fields_setup(consistent=projection == "consistent")
        if projection not in ("lumped", "consistent"):
            raise ValueError('fields: projection is "lumped" or "consistent"')
        names = species_names if species_names is not None else getattr(self, "species_names", None)
        pairs = [field_output.parse_request(r, self.model.n_species, self.n_eq, len(self.model.reactions), names)
                 for r in requests]
        return self._fields_call("fedm_fields", "fields", requests, pairs, t_out, t_old, t, projection, rtol, nodal, probes,
                                 max_it)

    # -- field output of LMEA models (csrc/gd_fields.hip) --------------------------------
    def gd_fields_setup(self, consistent=False):
        """:meth:`fields_setup` for an LMEA model (``fedm_gd_fields_setup``): what :meth:`gd_fields` needs once;
        ``consistent``: the P1 mass matrix of the plain measure as well.  Replaces an earlier set-up and drops its probe
        points."""
        if not isinstance(self.model, GdModel):
            raise RuntimeError("gd_fields: LMEA models only (fields() has the LFA family's)")
        mass = None
        if consistent:
            from . import amg, field_output
            keep = []
            mass = amg._csr_struct(field_output.mass_matrix(self._coords_dev, self._cells_dev), keep)
        self._check(self.lib.fedm_gd_fields_setup(self._h, C.byref(mass) if mass is not None else None),
                    "fedm_gd_fields_setup")
        self._fields_ready, self._n_probe_points = True, 0

    def gd_probe_setup(self, points):
        """:meth:`probe_setup` for an LMEA model (``fedm_gd_probe_setup``): probe points ``[n, 2]`` for
        :meth:`gd_fields`; a point on an edge or a vertex goes to the lowest cell index, a point outside the mesh is a
        ``ValueError`` naming it.  Returns ``(cells, weights)``."""
        from . import field_output
        if not isinstance(self.model, GdModel):
            raise RuntimeError("gd_fields: LMEA models only (fields() has the LFA family's)")
        if not getattr(self, "_fields_ready", False):
            self.gd_fields_setup()
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        cell, w = field_output.locate_points(self.coords, self.cells, pts)
        verts = np.ascontiguousarray(self._inv[self.cells[cell]], dtype=np.int32)
        w = np.ascontiguousarray(w)
        self._check(self.lib.fedm_gd_probe_setup(self._h, int(pts.shape[0]), verts.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 _dp(w)), "fedm_gd_probe_setup")
        self._n_probe_points = int(pts.shape[0])
        return cell, w

    def gd_fields(self, requests, t_out=None, t_old=None, t=None, projection="lumped", rtol=1e-10, nodal=True,
                  probes=False, max_it=10000, species_names=None):
        """Derived fields of an LMEA model from the resident state and the field table (``fedm_gd_fields``;
        include/fedm_hip.h has the definitions).  ``requests``: up to 8 names -- ``"state:e"``, ``"density:s"``,
        ``"charge"``, ``"mean_energy"`` (pointwise, from a state), ``"table:f"`` (a row of the field table), ``"E_r"``,
        ``"E_z"``, ``"E_norm"``, ``"reduced_field"`` (projected, from the potential), ``"rate:j"``, ``"source:s"``,
        ``"collision_loss"``, ``"joule"``, ``"flux_r:s"``, ``"flux_z:s"``, ``"current_r"``, ``"current_z"`` (projected, as
        the residual of the current step evaluates them) -- or ``(kind, index)`` pairs; ``s`` an index or one of
        ``species_names`` (the gas is 0; component 0 is the energy).  Times blend as in :meth:`fields`; the
        residual-evaluated kinds and ``table`` belong to the current step and take no ``t_out != t``.  Returns a
        :class:`FieldValues` in the caller's vertex order."""
        from . import field_output
        if not isinstance(self.model, GdModel):
            raise RuntimeError("gd_fields: LMEA models only (fields() has the LFA family's)")
        if projection not in ("lumped", "consistent"):
            raise ValueError('gd_fields: projection is "lumped" or "consistent"')
        if not getattr(self, "_fields_ready", False):
            self.gd_fields_setup(consistent=projection == "consistent")
        names = species_names if species_names is not None else getattr(self, "species_names", None)
        pairs = [field_output.parse_gd_request(r, self.model.n_species, self.model.n_reactions, self.model.n_fields, names)
                 for r in requests]
        return self._fields_call("fedm_gd_fields", "gd_fields", requests, pairs, t_out, t_old, t, projection, rtol, nodal,
                                 probes, max_it)

    def _fields_call(self, entry, what, requests, pairs, t_out, t_old, t, projection, rtol, nodal, probes, max_it):
        """One call of ``fedm_fields`` or ``fedm_gd_fields`` (``entry``) with the parsed ``pairs``."""
        if not 1 <= len(pairs) <= _lib.FIELDS_MAX_REQ:
            raise ValueError(f"{what}: 1 to {_lib.FIELDS_MAX_REQ} requests a call, got {len(pairs)}")
        req = (_lib.FieldReq * len(pairs))()
        for k, (kind, index) in enumerate(pairs):
            req[k].kind, req[k].index = kind, index
        opts = _lib.FieldOpts()
        if t_out is None:
            opts.num = opts.den = 1.0
        else:
            if t_old is None or t is None:
                raise ValueError(f"{what}: t_out goes with t_old and t")
            opts.num, opts.den = float(t_out) - float(t_old), float(t) - float(t_old)
        opts.projection, opts.max_it, opts.rtol = (1 if projection == "consistent" else 0), int(max_it), float(rtol)
        n_points = getattr(self, "_n_probe_points", 0)
        if probes and not n_points:
            raise RuntimeError(f"{what}: probes=True needs {'gd_' if what.startswith('gd_') else ''}probe_setup(points) first")
        out_n = np.empty((len(pairs), self.nv)) if nodal else None
        out_p = np.empty((len(pairs), n_points)) if probes else None
        finite = C.c_int32(0)
        its = (C.c_int32 * len(pairs))()
        import time
        t0 = time.perf_counter()
        rc = getattr(self.lib, entry)(self._h, C.byref(opts), len(pairs), req, _dp(out_n) if nodal else None,
                                         _dp(out_p) if probes else None, C.byref(finite), its)
        self.last_fields_call_seconds = time.perf_counter() - t0     # (the library's share; the rest is the reordering here)
        if rc == 3:
            raise RuntimeError(f"{entry}: conjugate gradients stopped at max_it = {max_it} "
                               f"(iterations per request {[int(v) for v in its]})")
        self._check(rc, entry)
        return FieldValues(names=[r if isinstance(r, str) else tuple(r) for r in requests],
                           # (np.take along the rows: five times faster than out_n[:, self._inv] at 341 k vertices)
                           nodal=np.take(out_n, self._inv, axis=1) if nodal else None, probes=out_p,
                           finite=bool(finite.value), cg_iterations=np.array([int(v) for v in its]))

    # -- Problem.F / Problem.J ------------------------------------------------
    def residual(self, download=True):
        F = np.empty(self.n) if download else None
        fn = C.c_double()
        self._check(self.lib.fedm_residual(self._h, _dp(F) if download else None, C.byref(fn)),
                    "fedm_residual")
        return (self._back(F), fn.value) if download else fn.value

    def jacobian(self):
        self._check(self.lib.fedm_jacobian(self._h), "fedm_jacobian")

    def residual_vector(self):
        """F as the last assembly left it (that of :meth:`residual` or the F + J of :meth:`jacobian`), not evaluated
        again."""
        F = np.empty(self.n)
        self._check(self.lib.fedm_get_residual(self._h, _dp(F)), "fedm_get_residual")
        return self._back(F)

    def jacobian_csr(self, device_order=False):
        """The assembled Jacobian as a scipy CSR matrix in the caller's dof numbering; ``device_order=True``: in the
        device's own (that of :meth:`fieldsplit_apply` and of the multigrid hierarchy)."""
        import scipy.sparse as sp
        nnz = self.lib.fedm_jacobian_nnz(self._h)
        indptr = np.empty(self.n + 1, dtype=np.int64)
        indices = np.empty(nnz, dtype=np.int32)
        values = np.empty(nnz)
        self._check(self.lib.fedm_jacobian_csr(
            self._h, indptr.ctypes.data_as(C.POINTER(C.c_int64)),
            indices.ctypes.data_as(C.POINTER(C.c_int32)), _dp(values)), "fedm_jacobian_csr")
        J = sp.csr_matrix((values, indices, indptr), shape=(self.n, self.n))
        if device_order:
            return J
        m = self._dof_new_of_old
        return J[m][:, m].tocsr()

    def spmv(self, x):
        x = self._vec(x)
        y = np.empty(self.n)
        self._check(self.lib.fedm_spmv(self._h, _dp(x), _dp(y)), "fedm_spmv")
        return self._back(y)

    def comm_roundtrip(self, vec, red=()):
        """One halo exchange of a DOF vector and one all-reduce through the context's transport
        (``fedm_debug_comm_roundtrip``): returns (vector with the ghost entries received, sums)."""
        x = self._vec(vec).copy()
        r = np.ascontiguousarray(red if len(red) else [0.0], dtype=np.float64).copy()
        self._check(self.lib.fedm_debug_comm_roundtrip(self._h, _dp(x), _dp(r), int(len(red))),
                    "fedm_debug_comm_roundtrip")
        return self._back(x), r[:len(red)]

    # -- multi-GPU transport ---------------------------------------------------------
    def _plan_arrays(self, lm):
        nb = np.ascontiguousarray(lm.neighbours, dtype=np.int32)
        sp_ = np.ascontiguousarray(lm.send_ptr, dtype=np.int32)
        si = np.ascontiguousarray(self._inv[lm.send_idx], dtype=np.int32)   # device numbering
        rp = np.ascontiguousarray(lm.recv_ptr, dtype=np.int32)
        self._plan_keep = (nb, sp_, si, rp)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        return len(nb), ip(nb), ip(sp_), ip(si), ip(rp)

    def init_comm_rccl(self, lm, unique_id: bytes, rank, n_ranks):
        """RCCL transport (ncclSend/ncclRecv halo groups + ncclAllReduce on the library's
        stream).  ``unique_id``: 128 bytes from :func:`rccl_unique_id` on rank 0."""
        uid = C.create_string_buffer(unique_id, 128)
        self._check(self.lib.fedm_comm_init_rccl(self._h, *self._plan_arrays(lm), uid,
                                                 int(rank), int(n_ranks)), "fedm_comm_init_rccl")

    def init_comm_torch(self, lm, group=None):
        """Host-staged transport through torch.distributed (gloo): the library copies the
        packed halo / the reduction scalars to pinned host memory and calls back here.
        Same algorithm as the RCCL path, used to test it where ranks share one GPU."""
        import torch
        import torch.distributed as dist
        n_send, n_ghost = int(lm.send_ptr[-1]), int(lm.recv_ptr[-1])

        def allreduce(buf, n, _user):
            a = np.ctypeslib.as_array(buf, shape=(n,))
            t = torch.from_numpy(a)
            dist.all_reduce(t, group=group)

        def exchange(send, recv, width, _user):
            s = np.ctypeslib.as_array(send, shape=(max(n_send, 1), width))
            r = np.ctypeslib.as_array(recv, shape=(max(n_ghost, 1), width))
            reqs, bufs = [], []
            for k, q in enumerate(lm.neighbours):
                out = torch.from_numpy(np.ascontiguousarray(s[lm.send_ptr[k]:lm.send_ptr[k + 1]]))
                reqs.append(dist.isend(out, int(q), group=group))
                buf = torch.empty((int(lm.recv_ptr[k + 1] - lm.recv_ptr[k]), width), dtype=torch.float64)
                bufs.append(buf)
                reqs.append(dist.irecv(buf, int(q), group=group))
            for q in reqs:
                q.wait()
            for k, buf in enumerate(bufs):
                r[lm.recv_ptr[k]:lm.recv_ptr[k + 1]] = buf.numpy()

        self._cb_keep = (_lib.ALLREDUCE_FN(allreduce), _lib.EXCHANGE_FN(exchange))
        self._check(self.lib.fedm_comm_init_callbacks(
            self._h, *self._plan_arrays(lm), self._cb_keep[0], self._cb_keep[1], None,
            dist.get_rank(group), dist.get_world_size(group)), "fedm_comm_init_callbacks")

    def sync_ghosts(self):
        self._check(self.lib.fedm_sync_ghosts(self._h), "fedm_sync_ghosts")

    def time_comm(self, kind, repeats=50):
        """ms per halo exchange (kind 0: block vector, 1: scalar) or all-reduce of 32 doubles (2)."""
        ms = C.c_double()
        self._check(self.lib.fedm_time_comm(self._h, int(kind), int(repeats), C.byref(ms)), "fedm_time_comm")
        return ms.value

    def comm_stats(self):
        """Transport kind and counters of the multi-GPU plumbing (``fedm_comm_stats``)."""
        out = (C.c_int64 * 10)()
        self._check(self.lib.fedm_comm_stats(self._h, out), "fedm_comm_stats")
        kind = {0: "none", 1: "host-staged callbacks", 2: "rccl"}[int(out[0])]
        return dict(transport=kind, ranks=int(out[1]), halo_exchanges=int(out[2]), allreduces=int(out[3]),
                    failed=bool(out[4]), neighbours=int(out[5]), interior_patches=int(out[6]),
                    boundary_patches=int(out[7]), halo_bytes=int(out[8]), allreduce_bytes=int(out[9]))

    # -- linear-solver set-up ---------------------------------------------------
    def block_csr(self, cr, cc):
        import scipy.sparse as sp
        nnz = self.lib.fedm_block_nnz(self._h)
        indptr = np.empty(self.nv + 1, dtype=np.int64)
        indices = np.empty(nnz, dtype=np.int32)
        values = np.empty(nnz)
        self._check(self.lib.fedm_block_csr(
            self._h, int(cr), int(cc), indptr.ctypes.data_as(C.POINTER(C.c_int64)),
            indices.ctypes.data_as(C.POINTER(C.c_int32)), _dp(values)), "fedm_block_csr")
        return sp.csr_matrix((values, indices, indptr), shape=(self.nv, self.nv))

    def setup_multigrid(self, theta=0.08, nu=2, omega=0.67, max_coarse=2000, max_sparse_levels=None,
                        poly_degree=None, poly_fraction=8.0, hard_poly_degree=None):
        """Build (host, once) and install the multigrid hierarchy of the constant potential
        block; afterwards Newton uses GMRES + field split (block Jacobi on the species,
        one V-cycle on the potential) and poisson_solve uses V-cycle-preconditioned CG.
        `poly_degree`: Chebyshev polynomial smoother of that many sweeps per leg instead of `nu`
        damped-Jacobi sweeps.  `hard_poly_degree`: such a cycle installed NEXT to the V(nu,nu)
        one, used with the alternative species sweeps of :meth:`set_fieldsplit` (one GPU)."""
        from . import amg
        if not self.model.poisson:
            raise ValueError("the model has no potential equation")
        self._check(self.lib.fedm_jacobian_poisson_only(self._h), "fedm_jacobian_poisson_only")
        ip = self.n_eq - 1
        K = self.block_csr(ip, ip)
        fixed = np.zeros(self.nv, dtype=bool)
        d = self._ddofs[self._ddofs % self.n_eq == ip] // self.n_eq
        fixed[d] = True            # device numbering, like K itself
        fixed[self.n_owned:] = True  # ghost rows are identity rows of the local block
        levels = amg.build_hierarchy(K, theta=theta, max_coarse=max_coarse, fixed=fixed,
                                     coords=self._coords_dev, max_sparse_levels=max_sparse_levels)
        self._last_hierarchy = levels
        if len(levels) < 2:                 # the whole block fits the dense coarsest solve: nothing to smooth
            poly_degree = hard_poly_degree = None
        if poly_degree:
            self.multigrid_levels = amg.install_poly(self._h, levels, poly_degree, poly_fraction)
        else:
            self.multigrid_levels = amg.install(self._h, levels, nu=nu, omega=omega)
        if hard_poly_degree:
            amg.install_poly(self._h, levels, hard_poly_degree, poly_fraction, alternative=True)
        return self.multigrid_levels

    def setup_multigrid_distributed(self, lm, group=None, theta=0.08, nu=1, omega=0.67, max_coarse=2000,
                                    prolongator_damping=4.0 / 3.0):
        """Several GPUs.  The potential block's multigrid is ONE global smoothed-aggregation
        hierarchy whose finest level is distributed and whose coarser levels are replicated:

        * aggregates are formed rank by rank (they never cross a partition boundary);
        * the prolongator is smoothed with the undecomposed operator: an owned vertex next to the
          boundary also interpolates from the neighbour's aggregates (the aggregate ids of the
          ghost vertices come from their owners), so constants are reproduced across ranks;
        * the level-1 operator is the sum of the ranks' contributions P_r^T K_r P (owned rows of K
          reach into ghost columns, whose prolongator rows come from the neighbours); every rank
          builds the hierarchy below it from the same matrix;
        * on the device the finest level is smoothed as a distributed operator (ghost values
          exchanged inside the V-cycle); its restriction writes straight into the global level-1
          vector, which is all-reduced once per cycle.

        With rank-local hierarchies (block Jacobi over ranks) GMRES needs 3x (2 ranks) to 4.5x
        (4 ranks) the single-GPU iterations.  The exchanges at set-up go through the process group."""
        import scipy.sparse as sp
        import torch.distributed as dist
        from . import amg
        if not self.model.poisson:
            raise ValueError("the model has no potential equation")
        self._check(self.lib.fedm_jacobian_poisson_only(self._h), "fedm_jacobian_poisson_only")
        ip = self.n_eq - 1
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        n_own, nv = lm.n_owned, self.nv
        to_dev, to_loc = self._inv, self._order            # local -> device index and back

        def from_neighbours(per_vertex):
            """Values of this rank's ghost vertices from their owners (list per neighbour);
            per_vertex is indexed by the partition's local vertex number."""
            send = {int(q): per_vertex[lm.send_idx[lm.send_ptr[k]:lm.send_ptr[k + 1]]]
                    for k, q in enumerate(lm.neighbours)}
            got = [None] * world
            dist.all_gather_object(got, send, group=group)
            return [got[int(q)][rank] for q in lm.neighbours]

        def gather(obj):
            out = [None] * world
            dist.all_gather_object(out, obj, group=group)
            return out

        # everything below in the partition's local numbering (owned vertices first)
        K = sp.csr_matrix(self.block_csr(ip, ip))[to_dev][:, to_dev]
        fixed = np.zeros(nv, dtype=bool)
        fixed[to_loc[self._ddofs[self._ddofs % self.n_eq == ip] // self.n_eq]] = True
        fixed[n_own:] = True
        diag = K.diagonal()
        for k, blk in enumerate(from_neighbours(diag)):     # ghost rows: their owners' diagonal
            diag[n_own + lm.recv_ptr[k]:n_own + lm.recv_ptr[k + 1]] = blk
        K = (K + sp.diags(diag - K.diagonal())).tocsr()
        step = amg.tentative_prolongator(K, theta, ~fixed, self.coords)
        if step is None:
            raise RuntimeError("multigrid coarsening of the finest level stalled")
        T, cxy = step                                        # n_local x n1 (ghost / fixed rows empty)
        n1 = T.shape[1]
        offset = np.concatenate([[0], np.cumsum(gather(int(n1)))]).astype(np.int64)
        n_g = int(offset[-1])
        # tentative prolongator with global columns, ghost rows filled from their owners
        agg = np.full(nv, -1, dtype=np.int64)
        Tc = T.tocoo()
        agg[Tc.row] = Tc.col + offset[rank]
        for k, blk in enumerate(from_neighbours(agg)):
            agg[n_own + lm.recv_ptr[k]:n_own + lm.recv_ptr[k + 1]] = blk
        has = agg >= 0
        T_ext = sp.csr_matrix((np.ones(int(has.sum())), (np.nonzero(has)[0], agg[has])), shape=(nv, n_g))
        # smoothed prolongator rows of the owned vertices: (I - w/rho D^-1 K) T with the whole K row
        DinvK = sp.diags(1.0 / diag[:n_own]) @ K[:n_own]
        rho = max(gather(float(np.abs(DinvK).sum(axis=1).max())))
        free_own = sp.diags((~fixed[:n_own]).astype(np.float64))
        P_own = (free_own @ (T_ext[:n_own] - (prolongator_damping / rho) * (DinvK @ T_ext))).tocsr()
        P_own.eliminate_zeros()
        # ... and of the ghost vertices, from their owners, for the Galerkin product
        P_ext = sp.vstack([P_own] + [sp.csr_matrix(blk) for blk in from_neighbours(P_own)]).tocsr() \
            if lm.n_ghost else P_own
        contribution = (P_own.T @ (K[:n_own] @ P_ext)).tocsr()            # n_g x n_g, sparse
        pieces = gather((contribution, cxy))
        A1 = pieces[0][0]
        for piece, _ in pieces[1:]:
            A1 = A1 + piece
        A1 = (0.5 * (A1 + A1.T)).tocsr()
        coords1 = np.vstack([c for _, c in pieces])
        # device: finest level (device numbering) with the global level-1 space as its coarse space
        R_dev = sp.vstack([P_own, sp.csr_matrix((nv - n_own, n_g))]).tocsr()[to_loc].T.tocsr()
        if self.halo_depth > 1:
            # deep halos: the correction P x_c is formed on the ghost layers too (their prolongator rows came
            # from the owners for the Galerkin product), so that the post-smoothing of the owned rows finds
            # exact neighbours without an exchange; the restriction sums OWNED rows only (each fine row once
            # over all ranks).  The outermost layer (identity rows) gets no correction.
            keep = np.ones(nv)
            keep[np.asarray(self._identity, dtype=np.int64)] = 0.0
            P_dev = (sp.diags(keep) @ P_ext).tocsr()[to_loc]
        else:
            P_dev = R_dev.T.tocsr()
        K_dev = K[to_loc][:, to_loc]
        local_sizes = amg.install(self._h, [(K_dev, P_dev), (A1, None)], nu=nu, omega=omega, dense_coarse=False,
                                  restrictions=[R_dev])
        levels_g = amg.build_hierarchy(A1, theta=theta, max_coarse=max_coarse, coords=coords1)
        global_sizes = amg.install_global(self._h, levels_g, n_g, 0, nu=nu, omega=omega)
        self.multigrid_levels = [local_sizes[0], f"{n1} of {n_g} global"] + global_sizes[1:]
        return self.multigrid_levels

    def set_fieldsplit(self, weights=(0.8, 0.8, 0.8), hard_weights=None, switch_above=5.0, back_below=3.5):
        """Richardson weights of the species-block sweeps; :func:`chebyshev_weights` gives the
        optimal ones for a spectrum interval of Duu^-1 Juu.  `hard_weights`: a second set (a cheaper
        one with the default species-first order, a higher degree with the potential-first order) used
        while Newton solves need >= `switch_above` Krylov steps per Newton iteration (until one
        needs <= `back_below` again)."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        self._check(self.lib.fedm_set_fieldsplit(self._h, int(w.size), _dp(w)), "fedm_set_fieldsplit")
        if hard_weights is not None:
            a = np.ascontiguousarray(hard_weights, dtype=np.float64)
            self._check(self.lib.fedm_set_fieldsplit_alternative(self._h, int(a.size), _dp(a),
                                                                 float(switch_above), float(back_below)),
                        "fedm_set_fieldsplit_alternative")

    def fieldsplit_policy(self):
        """Which preconditioner set ran (``fedm_fieldsplit_policy``): policy, active set, solves under each."""
        out = (C.c_int64 * 4)()
        self._check(self.lib.fedm_fieldsplit_policy(self._h, out), "fedm_fieldsplit_policy")
        return dict(policy="measured (wall time per Newton iteration)" if out[0] else "Krylov counts",
                    alternative_active=bool(out[1]), solves_main_set=int(out[2]), solves_alternative_set=int(out[3]))

    def clear_multigrid(self):
        self.lib.fedm_amg_clear(self._h)

    # -- solves --------------------------------------------------------------
    def newton_solve(self, rtol=1e-9, max_it=50, atol=1e-10, stol=1e-16,
                     ksp_restart=30, ksp_rtol=1e-5, ksp_atol=1e-50, ksp_max_it=10000):
        # (watch_component: the field whose relative change adaptive_solver asks for right after
        # the solve -- its two sums then ride on the final residual check's publication)
        watch = getattr(self, "watch_component", None)
        o = _lib.NewtonOpts(rtol, atol, stol, max_it, ksp_restart, ksp_rtol, ksp_atol, ksp_max_it,
                            0 if watch is None else int(watch) + 1)
        r = _lib.NewtonReport()
        if self._photo_stale:      # the source of this step, from the accepted state u_old; a retried step keeps it
            self.photo_update()
        rc = self.lib.fedm_newton_solve(self._h, C.byref(o), C.byref(r))
        self.last_report = NewtonReport(r.iterations, bool(r.converged), r.linear_iterations,
                                        r.fnorm0, r.fnorm)
        self._check(rc, "fedm_newton_solve")
        self._layers_solved = True     # (accept_layers: there is a solved step to accept)
        return r.iterations, True

    def poisson_solve(self, rtol=1e-10, max_it=20000):
        its = C.c_int()
        self._check(self.lib.fedm_poisson_solve(self._h, float(rtol), int(max_it), C.byref(its)),
                    "fedm_poisson_solve")
        return its.value

    # -- segregated (uncoupled) step: the potential with the densities frozen, then the species with the field frozen
    def poisson_update(self, rtol=1e-10, max_it=20000):
        """The potential entries of ``u_new`` from the Poisson rows with its species entries frozen
        (``fedm_poisson_update``; the reference's ``Poisson_solver``).  Returns the CG iterations, kept in
        ``last_poisson_iterations`` too."""
        its = C.c_int()
        rc = self.lib.fedm_poisson_update(self._h, float(rtol), int(max_it), C.byref(its))
        self.last_poisson_iterations = its.value
        self._check(rc, "fedm_poisson_update")
        return its.value

    def newton_solve_species(self, rtol=1e-9, max_it=50, atol=1e-10, stol=1e-16,
                             ksp_restart=30, ksp_rtol=1e-5, ksp_atol=1e-50, ksp_max_it=10000):
        """Newton on the species rows with the potential entries frozen (``fedm_newton_solve_species``).
        ``last_report`` carries its counts and its norms over the species entries."""
        o = _lib.NewtonOpts(rtol, atol, stol, max_it, ksp_restart, ksp_rtol, ksp_atol, ksp_max_it, 0)
        r = _lib.NewtonReport()
        rc = self.lib.fedm_newton_solve_species(self._h, C.byref(o), C.byref(r))
        self.last_report = NewtonReport(r.iterations, bool(r.converged), r.linear_iterations,
                                        r.fnorm0, r.fnorm)
        self._check(rc, "fedm_newton_solve_species")
        return r.iterations, True

    def species_assembly(self, jacobian=True):
        """Test hook: the assembly of one species Newton iteration alone (``fedm_debug_species_assembly``): F_u and
        J_uu, or with ``jacobian=False`` F_u by the residual-only twin.  True when the species-only one-pass kernel
        ran, False when the full assembly did."""
        rc = self.lib.fedm_debug_species_assembly(self._h, 1 if jacobian else 0)
        if rc < 0:
            self._check(rc, "fedm_debug_species_assembly")
        return bool(rc)

    def block_product(self, which, x):
        """Test hook: ``y = J_bb x_b`` with the Jacobian as it stands, ``which`` = "species" or "potential"
        (``fedm_debug_block_product``); caller's dof order, exact zeros on the other block's entries."""
        x = self._vec(x)
        y = np.empty(self.n)
        self._check(self.lib.fedm_debug_block_product(self._h, {"species": 0, "potential": 1}[which], _dp(x), _dp(y)),
                    "fedm_debug_block_product")
        return self._back(y)

    def species_linear_solve(self, b, ksp_restart=30, ksp_rtol=1e-5, ksp_atol=1e-50, ksp_max_it=10000):
        """Test hook: flexible GMRES on ``J_uu x_u = b_u`` with the Jacobian as the last species assembly left it,
        through the call the species Newton makes (``fedm_debug_species_linear_solve``).  Returns
        ``(x, its, rnorm, code)``: x with zeros on the potential entries, the step count, the true residual norm the
        solver reports and its return code (0 or FEDM_DIVERGED_*)."""
        o = _lib.NewtonOpts(0.0, 0.0, 0.0, 0, ksp_restart, ksp_rtol, ksp_atol, ksp_max_it, 0)
        b = self._vec(b)
        x = np.zeros(self.n)
        its, rnorm = C.c_int(), C.c_double()
        rc = self.lib.fedm_debug_species_linear_solve(self._h, _dp(b), C.byref(o), _dp(x), C.byref(its),
                                                      C.byref(rnorm))
        if rc < 0:
            self._check(rc, "fedm_debug_species_linear_solve")
        return self._back(x), its.value, rnorm.value, rc

    def segregated_solve(self, poisson_rtol=1e-10, poisson_max_it=20000, **newton):
        """One segregated step from the state as it stands: ``poisson_update`` then ``newton_solve_species``
        (whose arguments ``newton`` holds).  First order in dt against ``newton_solve``; explicit in the space
        charge, so stable for ``dt < eps0 / (e mu_e n_e)``."""
        self.poisson_update(rtol=poisson_rtol, max_it=poisson_max_it)
        return self.newton_solve_species(**newton)

    SEGREGATED_STATS = ("poisson_updates", "cg_iterations", "species_solves", "one_pass_assemblies",
                        "fallback_assemblies", "newton_iterations", "krylov_steps", "reserved")

    def segregated_stats(self, reset=False):
        """Counters of the segregated step since the context was created or they were last reset
        (``fedm_segregated_stats``), by name."""
        out = (C.c_int64 * 8)()
        self._check(self.lib.fedm_segregated_stats(self._h, out, 1 if reset else 0), "fedm_segregated_stats")
        return dict(zip(self.SEGREGATED_STATS, (int(v) for v in out)))

    def field_error(self, component):
        e = C.c_double()
        self._check(self.lib.fedm_field_error(self._h, int(component), C.byref(e)), "fedm_field_error")
        return e.value

    def plane_masks(self):
        """(kept, zero): bit masks over the n_eq x n_eq value planes of a Jacobian block that the
        assembly keeps between assemblies / that the SpMV skips (``fedm_plane_masks``)."""
        kept, zero = C.c_uint32(), C.c_uint32()
        self._check(self.lib.fedm_plane_masks(self._h, C.byref(kept), C.byref(zero)), "fedm_plane_masks")
        return kept.value, zero.value

    def set_assembly(self, kind):
        """'patch' (LDS patches, default) or 'colour' (global colouring, bitwise reproducible)."""
        code = {"colour": 0, "patch": 1}[kind]
        self._check(self.lib.fedm_set_assembly(self._h, code), "fedm_set_assembly")

    def set_preconditioner_side(self, side):
        """'right' (flexible GMRES, true residual norm; default for LFA models) or 'left'
        (preconditioned residual norm; default for LMEA models)."""
        code = {"left": 0, "right": 1}[side]
        self._check(self.lib.fedm_set_preconditioner_side(self._h, code), "fedm_set_preconditioner_side")

    def set_fieldsplit_order(self, order):
        """'lower' (default: species first; the true residual tracks the error of the iterate) or
        'upper' (V-cycle on the potential block first, species sweeps on the residual minus
        J_u,phi z_phi: the residual test passes in half the Krylov steps late in a streamer run, but
        the potential is left at V-cycle accuracy -- include/fedm_hip.h); order of the
        block-triangular split when it is on the right of the operator.  Takes effect with the next
        Jacobian assembly.  With ``set_krylov_scaling("rows")`` that caveat no longer holds: the
        equilibrated residual norm sees the Poisson rows, and a converged solve means the same accuracy
        in either order."""
        code = {"lower": 0, "upper": 1}[order]
        self._check(self.lib.fedm_set_fieldsplit_order(self._h, code), "fedm_set_fieldsplit_order")

    def set_krylov_scaling(self, mode):
        """'none' (default: GMRES tests ``|b - J x|``, which the species rows dominate) or 'rows': GMRES minimises
        and tests ``|D (b - J x)|`` against ``max(ksp_rtol |D b|, ksp_atol)`` with ``d_i`` one over the 2-norm of row
        ``i`` of its vertex's diagonal block (1 for identity rows), so that every equation is held on its own scale
        (``fedm_set_krylov_scaling``).  Field split on the right only: a solve under point-block Jacobi or with the
        split on the left raises.  The Newton loop's own test stays on the unscaled ``|F|``."""
        code = {"none": 0, "rows": 1}[mode]
        self._check(self.lib.fedm_set_krylov_scaling(self._h, code), "fedm_set_krylov_scaling")

    def krylov_scaling_mode(self):
        """0 (none) or 1 (rows): the mode alone, without the vector."""
        mode = C.c_int()
        self._check(self.lib.fedm_get_krylov_scaling(self._h, C.byref(mode), None), "fedm_get_krylov_scaling")
        return mode.value

    def krylov_scaling(self):
        """``(mode, d)``: 0 or 1, and the row scaling ``d`` of the Jacobian as it stands (what a scaled solve started now
        uses; caller's dof order) -- ``fedm_get_krylov_scaling``."""
        mode = C.c_int()
        d = np.empty(self.n)
        self._check(self.lib.fedm_get_krylov_scaling(self._h, C.byref(mode), _dp(d)), "fedm_get_krylov_scaling")
        return mode.value, self._back(d)

    # -- measurement ----------------------------------------------------------
    def species_planes_check(self):
        """Test hook: the field split's planes as they stand against the separate pass over the Jacobian as it stands:
        (relative difference of Duu^-1, absolute of the half-precision species planes, relative of the coupling plane,
        whether the last set-up was the one fused into the assembly)."""
        out = (C.c_double * 4)()
        self._check(self.lib.fedm_debug_species_planes_check(self._h, out), "fedm_debug_species_planes_check")
        return float(out[0]), float(out[1]), float(out[2]), bool(out[3])

    def time_kernel(self, kind, repeats=20):
        ms = C.c_double()
        self._check(self.lib.fedm_time_kernel(self._h, int(kind), int(repeats), C.byref(ms)),
                    "fedm_time_kernel")
        return ms.value

    def profile(self, enable=True):
        """True / 1: time the assembly kernels only (the solver is untouched).  2: also time the
        Jacobian SpMV and the V-cycle -- GMRES then launches kernel by kernel instead of
        replaying its per-iteration graphs, so use it for a separate profiling pass."""
        self._check(self.lib.fedm_profile(self._h, int(enable)), "fedm_profile")

    def profile_read(self):
        """{kind: (total ms, launches)} of the kernels timed since profile(True)."""
        names = {0: "assembly_FJ", 1: "spmv", 2: "assembly_F", 3: "vcycle"}
        out = {}
        for k, name in names.items():
            ms, cnt = C.c_double(), C.c_int64()
            self._check(self.lib.fedm_profile_read(self._h, k, C.byref(ms), C.byref(cnt)),
                        "fedm_profile_read")
            out[name] = (ms.value, cnt.value)
        return out

    def gd_assembly_kernel_name(self):
        """The LMEA F + J assembly kernels in use (bench.py's glow-discharge roofline block)."""
        return ("gd_jacobian_rows_kernel<.., BALL> + gd_gather_dest_rows_kernel (hand-derived element blocks of all cells, the "
                "three column vertices side by side at one wave per SIMD; summed per stored matrix position and row; F + J)")

    def sizes(self):
        v = [C.c_int64() for _ in range(6)]
        self.lib.fedm_sizes(self._h, *[C.byref(x) for x in v])
        keys = ("n_vertices", "n_cells", "n_eq", "nnz_blocks", "stored_blocks", "n_colours")
        out = dict(zip(keys, (x.value for x in v)))
        kept, zero = self.plane_masks()
        out["kept_planes"], out["zero_planes"] = bin(kept).count("1"), bin(zero).count("1")
        info = (C.c_int64 * 9)()
        self._check(self.lib.fedm_pattern_info(self._h, info), "fedm_pattern_info")
        out.update(zip(("n_slices", "max_patch_cells", "max_patch_width", "max_patch_verts", "cell_visits",
                        "halo_vertices"), (int(v) for v in info[:6])))
        out["assembly_variant"] = _VARIANTS[int(info[6])]
        out["patch_threads"] = int(info[7])
        out["model_structure"] = "compiled in" if info[8] else "run time"
        return out

    def assembly_variant(self):
        return self.sizes()["assembly_variant"]

    def launched_assembly(self):
        """The volume-assembly kernels the last residual-only assembly ("residual") and the last Jacobian assembly
        ("jacobian") launched (``fedm_launched_assembly``): variant (as :meth:`assembly_variant` names it; None before
        the first), threads per workgroup, launches and workgroups of all launches."""
        out = (C.c_int64 * 8)()
        self._check(self.lib.fedm_launched_assembly(self._h, out), "fedm_launched_assembly")
        rec = {}
        for k, what in enumerate(("residual", "jacobian")):
            v, threads, launches, wgs = (int(x) for x in out[4 * k:4 * k + 4])
            rec[what] = dict(variant=_VARIANTS[v] if v >= 0 else None, threads=threads, launches=launches,
                             workgroups=wgs)
        return rec

    def solver_path_stats(self, reset=False):
        """Which branches of the GMRES driver and of the Newton loop have run on this context
        (``fedm_solver_path_stats``; host counters, named as :data:`SOLVER_PATH_STATS`); ``reset=True`` zeroes them
        after reading."""
        out = (C.c_int64 * 24)()
        self._check(self.lib.fedm_solver_path_stats(self._h, out, int(bool(reset))), "fedm_solver_path_stats")
        return {name: int(out[k]) for k, name in enumerate(SOLVER_PATH_STATS)}

    def linear_solve(self, b, ksp_restart=30, ksp_rtol=1e-5, ksp_atol=1e-50, ksp_max_it=10000):
        """Test hook: GMRES on ``J x = b`` with the Jacobian of the last :meth:`jacobian` / :meth:`newton_solve`, through
        the call the Newton loop makes (``fedm_debug_linear_solve``).  Returns ``(x, its, rnorm, code)`` with the
        solver's own return code (0, or a key of ``_lib.DIVERGED``) instead of raising on a numerical failure; b and x
        in the caller's dof order.  The state is untouched; :meth:`residual_vector` is -b afterwards."""
        b = self._vec(b)
        x = np.empty(self.n)
        o = _lib.NewtonOpts(0.0, 0.0, 0.0, 0, ksp_restart, ksp_rtol, ksp_atol, ksp_max_it, 0)
        its, rn = C.c_int(), C.c_double()
        rc = self.lib.fedm_debug_linear_solve(self._h, _dp(b), C.byref(o), _dp(x), C.byref(its), C.byref(rn))
        if rc < 0:
            self._check(rc, "fedm_debug_linear_solve")
        return self._back(x), its.value, rn.value, rc

    def fieldsplit_apply(self, t):
        """z = Minv t with the field split of the current Jacobian (test hook; call jacobian() first).  t and z are in
        the device's vertex numbering (:meth:`jacobian_csr` with ``device_order=True``), not the caller's."""
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        assert t.size == self.n
        z = np.empty(self.n)
        self._check(self.lib.fedm_debug_fieldsplit_apply(self._h, _dp(t), _dp(z)), "fedm_debug_fieldsplit_apply")
        return z

    def fieldsplit_apply_operator(self, v):
        """(t, z) = (J v, Minv J v) as a Krylov step of the left-preconditioned GMRES forms them (the operator Minv J):
        the Jacobian product with the field split's first stage in its epilogue, then the rest of the preconditioner
        (test hook; call jacobian() first; lower-triangular order).  Like :meth:`fieldsplit_apply`, vectors in the
        device's numbering."""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        assert v.size == self.n
        t, z = np.empty(self.n), np.empty(self.n)
        self._check(self.lib.fedm_debug_fieldsplit_apply_operator(self._h, _dp(v), _dp(t), _dp(z)),
                    "fedm_debug_fieldsplit_apply_operator")
        return t, z

    def fieldsplit_apply_produced(self, t, coef):
        """(y, z = Minv y) as a Krylov step of the right-preconditioned GMRES forms them on one GPU with species sweeps:
        the kernel that completes the Krylov vector y forms the preconditioner's first stage as well.  ``coef`` of
        length 1: y = coef[0] t (the vector scaling); of length k + 1: y = (t - sum_i coef[i] t) coef[k] (the
        Gram-Schmidt update over k basis vectors).  Test hook; vectors in the device's numbering."""
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        cf = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
        assert t.size == self.n and 1 <= cf.size <= 9
        y, z = np.empty(self.n), np.empty(self.n)
        self._check(self.lib.fedm_debug_fieldsplit_apply_produced(self._h, _dp(t), int(cf.size - 1), _dp(cf), _dp(y),
                                                                  _dp(z)), "fedm_debug_fieldsplit_apply_produced")
        return y, z

    def krylov_op(self, op, k=0, V=None, y=None, x=None, x0=None, coef=None, red=None, finish=0, y_index=-1, slot=0,
                  a=1.0, sentinel=1e30):
        """Test hook: ONE launch wrapper of a Krylov step's reductions and vector updates on the caller's vectors
        (``fedm_debug_krylov_op``; ``op`` a key of ``_lib.KRYLOV_OPS``, the fields each op reads are listed in
        include/fedm_hip.h).  Vectors in the device's numbering: ``V`` of shape (n_vec, n), ``y`` and ``x`` of n
        entries, ``x0`` of n_vertices.  ``red``: the two reduction rows, shape (2, 40), uploaded before the op when
        given.  Every device entry outside the part of a vector that takes part in reductions holds ``sentinel``.
        Returns a dict: ``y`` and ``x`` as the op left them, ``red`` (2, 40), ``mail`` (the published slot, or None),
        ``published``, ``host_seq`` and ``device_seq`` (the publication counts), ``allocated`` (the Krylov storage was
        made by this call), and for the ops with the field split's first stage ``g32`` (n_vertices, 2) and ``b0``."""
        io = _lib.KrylovIo()
        keep = []

        def arr(v, size, what):
            if v is None:
                return None
            v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
            if v.size != size:
                raise ValueError(f"krylov_op: {what} must have {size} entries, got {v.size}")
            keep.append(v)
            return _dp(v)

        n_vec = 0 if V is None else int(np.asarray(V).shape[0])
        io.n_vec, io.finish, io.y_index, io.slot = n_vec, int(finish), int(y_index), int(slot)
        io.a, io.sentinel = float(a), float(sentinel)
        io.V = arr(V, n_vec * self.n, "V") if n_vec else None
        io.y, io.x, io.x0 = arr(y, self.n, "y"), arr(x, self.n, "x"), arr(x0, self.nv, "x0")
        io.coef = arr(coef, max(int(k), 0), "coef")
        red_io = np.zeros((2, _lib.KOP_RED_K))
        if red is not None:
            red_io[...] = np.asarray(red, dtype=np.float64).reshape(2, _lib.KOP_RED_K)
            io.red_in = 1
        y_out, x_out, mail = np.empty(self.n), np.empty(self.n), np.empty(_lib.KOP_RED_K)
        g32, b0 = np.empty((self.nv, 2), dtype=np.float32), np.empty(self.nv)
        io.red, io.y_out, io.x_out, io.mail, io.b0 = _dp(red_io), _dp(y_out), _dp(x_out), _dp(mail), _dp(b0)
        io.g32 = g32.ctypes.data_as(C.POINTER(C.c_float))
        self._check(self.lib.fedm_debug_krylov_op(self._h, _lib.KRYLOV_OPS[op], int(k), C.byref(io)),
                    "fedm_debug_krylov_op")
        published = int(io.info[0])
        fs = op in ("cgs_update_fs", "scale_copy_fs", "cgs_refine")
        return dict(y=y_out, x=x_out, red=red_io, mail=mail if published > 0 else None, published=published,
                    host_seq=int(io.info[1]), device_seq=int(io.info[2]), allocated=bool(io.info[3]),
                    g32=g32 if fs else None, b0=b0 if fs else None)

    def configure_fieldsplit_tiles(self, on, slices_per_tile=0, layers=0, threads=0, multigrid=True):
        """Test hook: species sweeps on tiles (several per launch) or one launch each; multigrid=False keeps the
        finest multigrid level's sweeps as kernels of their own."""
        mode = (1 if on else 0) | (0 if multigrid else 2)
        self._check(self.lib.fedm_debug_fieldsplit_tiles(self._h, mode, int(slices_per_tile), int(layers),
                                                         int(threads)), "fedm_debug_fieldsplit_tiles")

    def fieldsplit_tiles(self):
        """How the species sweeps of the field split run here: None = one launch per sweep; else the tiles of
        csrc/fs_tiles.hip (several sweeps per launch, the vertex layers around a tile of slices in LDS)."""
        info = (C.c_int64 * 10)()
        rc = self.lib.fedm_fieldsplit_tiles_info(self._h, info)
        if rc < 0:
            self._check(rc, "fedm_fieldsplit_tiles_info")
        if rc == 0:
            return None
        return dict(zip(("n_tiles", "slices_per_tile", "layers", "row_width", "max_vertices", "max_rows", "bytes",
                         "threads", "total_rows", "total_vertices"), (int(v) for v in info[:10])))


def rccl_unique_id():
    """128-byte ncclUniqueId (call on one rank, broadcast to the others)."""
    buf = C.create_string_buffer(128)
    lib = _lib.load()
    if lib.fedm_comm_unique_id(buf) != 0:
        raise RuntimeError(f"fedm_comm_unique_id failed: {_lib.last_error()}")
    return buf.raw


def chebyshev_weights(m, lam_min=0.5, lam_max=2.0):
    """Richardson weights whose residual polynomial is the degree-m Chebyshev polynomial on
    [lam_min, lam_max] (defaults: the diagonally scaled P1 mass matrix in 2-D)."""
    theta, delta = 0.5 * (lam_max + lam_min), 0.5 * (lam_max - lam_min)
    k = np.arange(1, m + 1)
    return 1.0 / (theta + delta * np.cos((2 * k - 1) * np.pi / (2 * m)))
