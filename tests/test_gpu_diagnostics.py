"""Discharge diagnostics on the device (csrc/diag.hip, DeviceProblem.diagnostics) against the numpy restatement of
tests/diagnostics_reference.py, which tests/test_diagnostics_reference.py pins on closed forms.

Meshes of the streamer box: (a) 3 x 3 -- 18 cells, less than one wave; (b) 12 x 17 -- 408 cells, two workgroups, the
second partly empty, not square; (c) the graded Delaunay mesh of test_gpu_photoionization.py, whose device numbering
moves most vertices; (d) 182 x 182 -- 66 248 cells, more than DIAG_BLOCKS x DIAG_THREADS = 256 x 256 = 65 536, so the
cell pass's stride loop runs (the second pass never loops: the first writes at most 256 partials per slot).
States: the oracle's initial streamer state with photoionization_reference.perturbed, u_new != u_old.  Models: the
closed-form streamer, axisymmetric and planar; its tabulated twin with quantile_knots; lfa_models.four_species_problem
(NS = 4, a drifting ion, a prescribed drift); a one-species model without a Poisson equation; the linear-representation
model of test_oracle_linear.py (test_gpu_parity.py's).  psi = z / BOX + 0.2 (r / BOX)^2 has both gradient components.

Bounds.  Sums: |device - fsum| <= 1e-12 sum |terms| (the summation tree is about 20 levels deep, a few 1e-15 of
sum |terms|; a term's own error is dominated by exp(u), |u| <~ 45, about 1e-14 relative; 1e-12 leaves two orders over
that and is one order tighter than the 1e-11 F is held to).  Field maxima 1e-13 relative, index and centroid exact where
the restatement's maximum is unique.  Nodal maxima bitwise.  Ranks: check 1's bound on the global sum |terms|, maxima
to 4 eps with the same global cell and vertex.

MEASURED on the MI355X (every test prints its figures before it asserts).  Worst |device - fsum| / sum |terms|: meshes
(a)-(d), closed / planar / tabulated 1.1e-15 (typical 1e-16 .. 9e-16), four species 4.7e-16, linear representation and
the model without a Poisson equation below 1e-15; state "old" the same; the ranks' shares against the restatement
1.6e-15 and against the one-GPU call 1.5e-16 (r-cut, z-cut, three-way, depths 1 and 8, both models); two processes
through Runner.diagnose 4.0e-15; the example's two rows 2.0e-15.  Field maxima: 0 .. 1.7e-15 relative, cell and
centroid those of the restatement in every planted case.  Nodal maxima bitwise.  The whole file runs in about 10 s, no
test above 3 s.
"""
import dataclasses
import importlib.util
import math
import os
import socket
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import diagnostics_reference as dref  # noqa: E402
import photoionization_reference as pr  # noqa: E402
import rank_assembly_reference as rr  # noqa: E402
import tabulated_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps
SUM_BOUND, MAX_BOUND = 1e-12, 1e-13
WINDOW_FRACTIONS = (0.0, 0.35, 0.2, 1.0)        # of the box: r_lo, r_hi, z_lo, z_hi
TENSOR = {"a": (3, 3), "b": (12, 17), "d": (182, 182)}


def _mesh(name):
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh, rectangle_right
    if name in TENSOR:
        m = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, *TENSOR[name])
        assert m.nc == 2 * TENSOR[name][0] * TENSOR[name][1]
        return m
    from fedm_amd import meshgen
    size = meshgen.box_distance_size((0.0, 1.5e-3, 7e-3, 11e-3), 3e-4, 0.6, 3e-3)
    g = meshgen.refined_rectangle(ost.BOX, ost.BOX, size, 3e-4, n_levels=3)
    assert 200 <= g.coords.shape[0] <= 700
    return OMesh(g.coords, g.cells)


def _window():
    from oracle import streamer as ost
    return tuple(f * ost.BOX for f in WINDOW_FRACTIONS)


def _psi(coords):
    from oracle import streamer as ost
    return coords[:, 1] / ost.BOX + 0.2 * (coords[:, 0] / ost.BOX) ** 2


def _electrodes(coords):
    from oracle import streamer as ost
    z = coords[:, 1]
    return np.where(np.abs(z) < 3e-16, 1, np.where(np.abs(z - ost.BOX) < 3e-16, 2, 0)).astype(np.int8)


def _models(mesh, kind):
    """(oracle model, device Model, U_new, U_old) of a two-species streamer variant."""
    from oracle import streamer as ost
    from fedm_amd.cases import streamer
    plain = ost.build(mesh)
    U0 = ost.initial_state(plain)
    U_old, U_new = pr.perturbed(U0, 21), pr.perturbed(U0, 22)
    if kind == "tabulated":
        x = tr.quantile_knots(plain.cell_fields(U_new)[2])
        om, dm = tr.oracle_streamer(mesh, x), tr.device_streamer_model(x)
        if mesh.nc > 100:
            tr.assert_knots_exercise_the_lookup(x, om.cell_fields(U_new)[2])
    else:
        om, dm = plain, streamer.model()
    if kind == "planar":
        om.axisymmetric = False
        om._geometry()
        dm = dataclasses.replace(dm, axisymmetric=False)
    return om, dm, U_new, U_old


class Case:
    """One (mesh, model): the oracle model, the states, the restatement (computed once, never changed) and one device
    problem with psi and the electrode groups set up."""

    def __init__(self, mesh_name, kind):
        self.mesh = _mesh(mesh_name)
        self.om, dm, self.U_new, self.U_old = _models(self.mesh, kind)
        self.psi, self.group, self.window = _psi(self.mesh.coords), _electrodes(self.mesh.coords), _window()
        self.prob = tr.device_streamer_problem(self.mesh.coords, self.mesh.cells, dm)
        self.prob.set_state(self.U_new, self.U_old, self.U_old)
        self.prob.diagnostics_setup(weighting_potential=self.psi, vertex_groups=self.group, n_groups=2)
        self._ref = {}

    def ref(self, which="new"):
        if which not in self._ref:
            U = self.U_new if which == "new" else self.U_old
            self._ref[which] = dref.reference(self.om, U, window=self.window, psi=self.psi, group=self.group, n_groups=2)
        return self._ref[which]

    def restate(self, U):
        return dref.reference(self.om, U, window=self.window, psi=self.psi, group=self.group, n_groups=2)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(mesh_name, kind="closed"):
        if (mesh_name, kind) not in made:
            made[mesh_name, kind] = Case(mesh_name, kind)
        return made[mesh_name, kind]
    yield get
    for c in made.values():
        c.prob.close()


def _check_sums(what, d, ref):
    """Every sum of one call against the restatement; prints the ratios to the bound first.  Returns the worst."""
    pairs = [(f"N[{s}]", d.species_integral[s], r) for s, r in enumerate(ref["species"])]
    pairs += [(f"q[{g}]", d.group_sum[g], r) for g, r in enumerate(ref["groups"])]
    pairs.append(("I_psi", d.induced_current, ref["current"]))
    ratios = {}
    for name, got, r in pairs:
        ratios[name] = abs(got - r.value) / r.abs if r.abs > 0.0 else (0.0 if got == 0.0 else math.inf)
    print(f"[diagnostics] {what}: |device - fsum| / sum|terms| " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()),
          flush=True)
    assert d.finite
    assert len(d.group_sum) == len(ref["groups"])
    for name, v in ratios.items():
        assert v <= SUM_BOUND, (what, name, v)
    return max(ratios.values())


def _check_maxima(what, d, ref):
    for name, value, cell, cen, r in (("field", d.field_max, d.field_max_cell, d.field_max_centroid, ref["field"]),
                                      ("window", d.window_max, d.window_max_cell, d.window_max_centroid, ref["window"])):
        print(f"[diagnostics] {what}: {name} max rel {abs(value - r.value) / max(r.value, 1e-300):.2e} cell {cell} "
              f"restated {r.index} unique {r.unique}", flush=True)
        if r.index < 0:
            assert value == 0.0 and cell == -1, (what, name)
            continue
        assert abs(value - r.value) <= MAX_BOUND * r.value, (what, name)
        if r.unique:
            assert cell == r.index and tuple(cen) == r.centroid, (what, name, cell, r.index, cen, r.centroid)


def _check_nodal(what, d, ref, U):
    for s, r in enumerate(ref["nodal"]):
        assert d.nodal_max[s] == r.value, (what, s)                   # bitwise a value of the state
        assert U[d.nodal_max_vertex[s], s] == r.value, (what, s)      # ... at the vertex named, caller's numbering
        if r.unique:
            assert d.nodal_max_vertex[s] == r.index, (what, s)


def _bytes(d):
    parts = [d.species_integral, d.group_sum, np.array([d.induced_current, d.field_max, d.window_max]),
             np.array(d.field_max_centroid), np.array(d.window_max_centroid), d.nodal_max,
             np.array([d.field_max_cell, d.window_max_cell, int(d.finite)]), d.nodal_max_vertex]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


# ---- 1: the sums (and, on the way, maxima and nodal maxima of the unplanted states) ------------------------------------
@pytest.mark.parametrize("mesh_name,kind", [("a", "closed"), ("b", "closed"), ("c", "closed"), ("d", "closed"),
                                            ("b", "planar"), ("c", "planar"), ("a", "tabulated"), ("b", "tabulated"),
                                            ("c", "tabulated"), ("d", "tabulated")])
def test_sums_against_the_restatement(cases, mesh_name, kind):
    c = cases(mesh_name, kind)
    d, ref = c.prob.diagnostics(window=c.window), c.ref()
    what = f"mesh ({mesh_name}) {kind}"
    _check_sums(what, d, ref)
    _check_maxima(what, d, ref)
    _check_nodal(what, d, ref, c.U_new)
    assert ref["current"].value != 0.0 and ref["groups"][0].abs > 0.0 and ref["groups"][1].abs > 0.0
    assert d.net_charge == d.species_integral[0] - d.species_integral[1]
    # without a window the second maximum is the first
    d2 = c.prob.diagnostics()
    assert (d2.window_max, d2.window_max_cell, d2.window_max_centroid) == (d2.field_max, d2.field_max_cell,
                                                                          d2.field_max_centroid)
    assert d2.field_max == d.field_max and d2.induced_current == d.induced_current


def test_four_species_with_drifting_ions():
    import lfa_models
    from fedm_amd.device import boundary_vertex_groups
    m, prob, om, _, _ = lfa_models.four_species_problem()
    try:
        from oracle import streamer as ost
        U2 = pr.perturbed(ost.initial_state(ost.build(om.mesh)), 22)
        r, z = m.coords[:, 0], m.coords[:, 1]
        rng = np.random.default_rng(31)
        bump = np.exp(-(r ** 2 + (z - 0.008) ** 2) / (2e-3) ** 2)
        U = np.column_stack([np.log(1e12 + 1e15 * bump) + rng.normal(0, 0.2, r.size), U2[:, 0],
                             np.log(1e11 + 1e14 * bump) + rng.normal(0, 0.2, r.size), U2[:, 1], U2[:, 2]])
        group = boundary_vertex_groups(m.cells, prob._tags, prob.nv, prob.dirichlet_vertices(), (1, 2))
        assert np.array_equal(group, _electrodes(m.coords))
        psi = _psi(m.coords)
        prob.set_state(U, U, U)
        prob.diagnostics_setup(weighting_potential=psi, vertex_groups=group)
        ref = dref.reference(om, U, window=_window(), psi=psi, group=group, n_groups=2)
        d = prob.diagnostics(window=_window())
        _check_sums("four species", d, ref)
        _check_maxima("four species", d, ref)
        _check_nodal("four species", d, ref, U)
        assert d.net_charge == pytest.approx(d.species_integral[1] - d.species_integral[2] - d.species_integral[3], rel=1e-15)
    finally:
        prob.close()


def test_one_species_without_a_poisson_equation():
    from oracle.forms import LFAModel, TermSum as OTermSum
    from oracle.mesh import mark_boundaries
    from oracle import streamer as ost
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum
    mesh = _mesh("b")
    k = [(3.0e7, 0.5, -2.0, 1.0)]
    om = LFAModel(mesh, n_species=1, poisson=False, eq_type=["diffusion-reaction"], Z=[-1.0], D=[0.1],
                  reactions=[(OTermSum(k), [1], [1])], facet_tags=mark_boundaries(mesh, ost.BOUNDARIES),
                  bc_type=[["zero flux"]] * 4, qdeg=2)
    dm = Model(n_species=1, poisson=False, eq_type=["diffusion-reaction"], Z=[-1.0], D=[TermSum.const(0.1)],
               reactions=[Reaction(TermSum(k), power=[1], net=[1])], bc_kind=[["zero flux"]] * 4, quadrature_degree=2)
    r, z = mesh.coords[:, 0], mesh.coords[:, 1]
    U = (np.log(1e13 + 1e17 * np.exp(-(r ** 2 + (z - 0.008) ** 2) / (2e-3) ** 2))
         + np.random.default_rng(31).normal(0, 0.2, mesh.nv))[:, None]
    msh = Mesh(mesh.coords, mesh.cells)
    prob = DeviceProblem(msh.coords, msh.cells, dm, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES))
    try:
        prob.set_state(U, U, U)
        with pytest.raises(RuntimeError, match="Poisson"):
            prob.diagnostics_setup(vertex_groups=_electrodes(mesh.coords))
        psi = _psi(mesh.coords)
        prob.diagnostics_setup(weighting_potential=psi)
        d = prob.diagnostics(window=_window())
        ref = dref.reference(om, U, window=_window(), psi=psi)
        _check_sums("one species, no Poisson equation", d, ref)
        _check_nodal("one species, no Poisson equation", d, ref, U)
        assert (d.field_max, d.field_max_cell, d.window_max, d.window_max_cell) == (0.0, -1, 0.0, -1)
        assert ref["current"].abs > 0.0                # the diffusive flux of a charged species
    finally:
        prob.close()


def test_linear_representation():
    from test_oracle_linear import _model, _state
    from fedm_amd.cases import streamer
    mesh = _mesh("b")
    om = _model(mesh, log=False)
    lnn, phi = _state(mesh, seed=9)
    U = np.column_stack([np.exp(lnn), phi])
    dm = dataclasses.replace(streamer.model(), log_representation=False)
    prob = tr.device_streamer_problem(mesh.coords, mesh.cells, dm)
    try:
        psi, group = _psi(mesh.coords), _electrodes(mesh.coords)
        prob.set_state(U, U, U)
        prob.diagnostics_setup(weighting_potential=psi, vertex_groups=group)
        d = prob.diagnostics(window=_window())
        ref = dref.reference(om, U, window=_window(), psi=psi, group=group, n_groups=2)
        _check_sums("linear representation", d, ref)
        _check_maxima("linear representation", d, ref)
        _check_nodal("linear representation", d, ref, U)
        assert np.array_equal(d.density_max, d.nodal_max)
    finally:
        prob.close()


# ---- 2: planted field maxima ---------------------------------------------------------------------------------------------
def _boundary_edge(mesh, cell):
    """Two vertices of `cell` whose edge no other cell has (None for an interior cell)."""
    c = mesh.cells
    for i, j in ((0, 1), (1, 2), (0, 2)):
        a, b = c[cell, i], c[cell, j]
        if ((c == a).any(axis=1) & (c == b).any(axis=1)).sum() == 1:
            return int(a), int(b)
    return None


def _plant(mesh, U, cell, amount, edge=None):
    """Phi raised at one end of an edge of `cell` and lowered at the other: the gradient grows most in the cells that
    hold the whole edge (one cell, for a boundary edge)."""
    V = U.copy()
    edge = edge or _boundary_edge(mesh, cell) or (int(mesh.cells[cell, 0]), int(mesh.cells[cell, 1]))
    V[edge[0], 2] += amount
    V[edge[1], 2] -= amount
    return V


def _plant_exactly(c, cell, amount):
    """(state, restatement) whose unique field maximum is `cell`: the first of the cell's edges and signs that does it
    (on the unstructured mesh a thin neighbour can outdo the cell for some of them)."""
    v = [int(i) for i in c.mesh.cells[cell]]
    first = _boundary_edge(c.mesh, cell)
    edges = ([first] if first else []) + [(v[i], v[j]) for i in range(3) for j in range(3) if i != j]
    for edge in edges:
        U = _plant(c.mesh, c.U_new, cell, amount, edge)
        ref = c.restate(U)
        if ref["field"].unique and ref["field"].index == cell:
            return U, ref
    raise AssertionError(f"no plant makes cell {cell} the maximum")


@pytest.mark.parametrize("mesh_name", ["a", "b", "c", "d"])
def test_planted_field_maxima(cases, mesh_name):
    c = cases(mesh_name)
    nc, cen = c.mesh.nc, dref.centroids(c.om)
    r_lo, r_hi, z_lo, z_hi = c.window
    inside = np.nonzero((cen[:, 0] >= r_lo) & (cen[:, 0] <= r_hi) & (cen[:, 1] >= z_lo) & (cen[:, 1] <= z_hi))[0]
    outside = np.setdiff1d(np.arange(nc), inside)
    interior = np.setdiff1d(inside, c.mesh.exterior_facets()[0])         # cells without a boundary edge
    assert inside.size and outside.size and interior.size
    mid = int(interior[len(interior) // 2])
    try:
        for what, cell in (("cell 0", 0), ("last cell", nc - 1), ("a mid cell", mid)):
            U, ref = _plant_exactly(c, cell, 5e6)
            c.prob.set_state(u_new=U)
            _check_maxima(f"mesh ({mesh_name}) planted at {what}", c.prob.diagnostics(window=c.window), ref)
        # the window's maximum is not the global one: a large plant outside, a smaller one inside
        far = int(outside[np.argmax(cen[outside, 0])])         # the cell farthest from the axis: no window cell near it
        U = _plant(c.mesh, _plant(c.mesh, c.U_new, far, 5e6), mid, 2e4)
        ref = c.restate(U)
        assert ref["field"].unique and ref["window"].unique and ref["field"].index != ref["window"].index
        assert ref["field"].value > 2.0 * ref["window"].value > 0.0
        c.prob.set_state(u_new=U)
        _check_maxima(f"mesh ({mesh_name}) window maximum below the global one", c.prob.diagnostics(window=c.window), ref)
        # an empty window
        d = c.prob.diagnostics(window=(2.0 * r_hi + 1.0, 3.0 * r_hi + 1.0, z_lo, z_hi))
        assert (d.window_max, d.window_max_cell, tuple(d.window_max_centroid)) == (0.0, -1, (0.0, 0.0))
        assert d.field_max_cell == ref["field"].index
        # a one-point window that holds exactly one centroid: closed on both sides
        k = int(inside[0])
        d = c.prob.diagnostics(window=(cen[k, 0], cen[k, 0], cen[k, 1], cen[k, 1]))
        assert d.window_max_cell == k and tuple(d.window_max_centroid) == (cen[k, 0], cen[k, 1])
    finally:
        c.prob.set_state(u_new=c.U_new)


# ---- 3: planted nodal maxima ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh_name", ["a", "c", "d"])
def test_planted_nodal_maxima(cases, mesh_name):
    c = cases(mesh_name)
    nv = c.mesh.nv
    moved = np.nonzero(c.prob._order != np.arange(nv))[0]       # vertices the device numbers differently
    other = int(moved[moved.size // 3]) if moved.size else nv // 3 + 1
    try:
        for s in range(2):
            for v in (0, nv - 1, other):
                U = c.U_new.copy()
                U[v, s] = 47.25 + s
                c.prob.set_state(u_new=U)
                d = c.prob.diagnostics()
                assert d.finite and d.nodal_max[s] == U[v, s] and d.nodal_max_vertex[s] == v, (mesh_name, s, v)
                t = 1 - s
                assert d.nodal_max[t] == c.U_new[:, t].max() and c.U_new[d.nodal_max_vertex[t], t] == d.nodal_max[t]
                assert d.density_max[s] == np.exp(U[v, s])
        # an exact tie: the lowest DEVICE vertex wins, and it comes back in the caller's numbering
        U = c.U_new.copy()
        tied = np.array([other, nv - 1, 1])
        U[tied, 1] = 46.5
        c.prob.set_state(u_new=U)
        d = c.prob.diagnostics()
        assert d.nodal_max[1] == 46.5 and d.nodal_max_vertex[1] == tied[np.argmin(c.prob._inv[tied])]
    finally:
        c.prob.set_state(u_new=c.U_new)
    if mesh_name == "c":
        assert (c.prob._order != np.arange(nv)).mean() > 0.5


# ---- 4: the state selector ------------------------------------------------------------------------------------------------
def test_state_selector_and_shift(cases):
    c = cases("c")
    new, old = c.prob.diagnostics(window=c.window, state="new"), c.prob.diagnostics(window=c.window, state="old")
    _check_sums("mesh (c) state old", old, c.ref("old"))
    _check_maxima("mesh (c) state old", old, c.ref("old"))
    _check_nodal("mesh (c) state old", old, c.ref("old"), c.U_old)
    assert _bytes(new) != _bytes(old)
    try:
        c.prob.shift_state()
        assert _bytes(c.prob.diagnostics(window=c.window, state="old")) == _bytes(new)
        assert _bytes(c.prob.diagnostics(window=c.window, state="new")) == _bytes(new)
    finally:
        c.prob.set_state(c.U_new, c.U_old, c.U_old)
    with pytest.raises(ValueError):
        c.prob.diagnostics(state="older")


# ---- 5, 6: reproducibility, and a state that is not finite ----------------------------------------------------------------
def test_two_calls_agree_byte_for_byte_and_a_nan_is_flagged(cases):
    c = cases("d")
    first = c.prob.diagnostics(window=c.window)
    assert _bytes(c.prob.diagnostics(window=c.window)) == _bytes(first)
    try:
        bad = c.U_new.copy()
        bad[c.mesh.nv // 2 + 5, 1] = np.nan
        c.prob.set_state(u_new=bad)
        d = c.prob.diagnostics(window=c.window)        # returns: the kernel reads and reduces the NaN, nothing faults
        assert d.finite is False
        bad = c.U_new.copy()
        bad[3, 2] = np.inf                              # ... and an infinite potential
        c.prob.set_state(u_new=bad)
        assert c.prob.diagnostics(window=c.window).finite is False
    finally:
        c.prob.set_state(u_new=c.U_new)
    again = c.prob.diagnostics(window=c.window)
    assert again.finite is True and _bytes(again) == _bytes(first)


# ---- 7: every rank of a partition, one context at a time -------------------------------------------------------------------
@pytest.fixture(scope="module")
def rank_setup():
    msh = rr.mesh()
    parts = rr.partitions(msh.coords, msh.cells)
    return dict(mesh=msh, parts=parts, cases={name: rr.CASES[name](msh) for name in ("streamer", "tabulated")})


def _create_rank(msh, lm, model):
    from fedm_amd.device import DeviceProblem
    dofs, vals = rr.local_dirichlet(lm, model.n_eq)
    return DeviceProblem(lm.coords, lm.cells, model, facet_tags=rr.local_facet_tags(msh, lm), dirichlet_dofs=dofs,
                         dirichlet_vals=vals, n_owned=lm.n_owned,
                         identity_vertices=lm.identity_vertices if lm.depth > 1 else None, halo_depth=lm.depth)


@pytest.mark.parametrize("partition", ["r-cut", "z-cut", "three"])
@pytest.mark.parametrize("model", ["streamer", "tabulated"])
def test_rank_shares_add_up_to_one_gpu(rank_setup, model, partition):
    msh, c = rank_setup["mesh"], rank_setup["cases"][model]
    om, U = c["om"], c["states"][0]
    psi, group, window = _psi(msh.coords), _electrodes(msh.coords), _window()
    ref = dref.reference(om, U, window=window, psi=psi, group=group, n_groups=2)
    assert ref["field"].unique and ref["window"].unique and all(n.unique for n in ref["nodal"])
    one = tr.device_streamer_problem(msh.coords, msh.cells, c["model"]())
    try:
        one.set_state(U, U, U)
        one.diagnostics_setup(weighting_potential=psi, vertex_groups=group)
        whole = one.diagnostics(window=window)
    finally:
        one.close()
    _check_sums(f"ranks: {model} on one GPU", whole, ref)
    names = ["N[0]", "N[1]", "q[0]", "q[1]", "I_psi"]
    refs = ref["species"] + ref["groups"] + [ref["current"]]
    whole_sums = [*whole.species_integral, *whole.group_sum, whole.induced_current]
    for depth in (1, 8):
        shares = []
        lms = rr.local_meshes(msh.coords, msh.cells, rank_setup["parts"][partition], depth)
        for lm in lms:
            prob = _create_rank(msh, lm, c["model"]())
            try:
                Ul = rr.restrict(lm, U)
                prob.set_state(Ul, Ul, Ul)
                prob.diagnostics_setup(weighting_potential=rr.restrict(lm, psi), vertex_groups=rr.restrict(lm, group),
                                       n_groups=2)
                d = prob.diagnostics(window=window)
                assert d.finite
                shares.append(d)
            finally:
                prob.close()
        what = f"ranks: {model} {partition} depth {depth}"
        got = [math.fsum(v) for v in zip(*[[*d.species_integral, *d.group_sum, d.induced_current] for d in shares])]
        ratios = [abs(g - r.value) / r.abs for g, r in zip(got, refs)]
        ratios_one = [abs(g - w) / r.abs for g, w, r in zip(got, whole_sums, refs)]
        print(f"[diagnostics] {what}: shares' fsum against the restatement " +
              " ".join(f"{n} {v:.2e}" for n, v in zip(names, ratios)) + " | against one GPU " +
              " ".join(f"{v:.2e}" for v in ratios_one), flush=True)
        assert max(ratios) <= SUM_BOUND and max(ratios_one) <= SUM_BOUND, what
        if partition == "r-cut":        # both electrode groups are split between the ranks
            assert all(d.group_sum[g] != 0.0 for d in shares for g in range(2))
        for key, value, cell in (("field", "field_max", "field_max_cell"), ("window", "window_max", "window_max_cell")):
            best = dref.combine_maxima([dref.Max(getattr(d, value), getattr(d, cell), True, None) for d in shares],
                                       [lm.cell_global for lm in lms])
            assert abs(best[0] - getattr(whole, value)) <= 4 * EPS * getattr(whole, value), (what, key)
            assert best[1] == getattr(whole, cell) == ref[key].index, (what, key)
        for s in range(2):
            best = dref.combine_maxima([dref.Max(d.nodal_max[s], int(d.nodal_max_vertex[s]), True, None) for d in shares],
                                       [lm.vertex_global for lm in lms])
            assert best == (whole.nodal_max[s], whole.nodal_max_vertex[s]) and best[1] == ref["nodal"][s].index, (what, s)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    from fedm_amd.cases import streamer_distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        run = streamer_distributed.Runner(None, rank, world, 0, grading=2.0, transport="torch", n_per_gpu=12)
        run.initialise()
        row = run.diagnose()
        q.put((rank, run.lm.vertex_global[:run.lm.n_owned], run.prob.get_state()[:run.lm.n_owned], row, run.global_n))
    finally:
        dist.destroy_process_group()


def test_runner_combines_two_ranks():
    """streamer_distributed.Runner.diagnose on two processes sharing the GPU over the host-staged transport: the
    combined row against the restatement applied to the glued state."""
    import mp_results
    import torch.multiprocessing as mp
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.cases import streamer
    from fedm_amd.physical_constants import elementary_charge, epsilon_0
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = mp_results.collect(procs, q, len(procs), 300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    msh = streamer.mesh(res[0][4], 2.0)
    U = np.zeros((msh.coords.shape[0], 3))
    for _, gids, Uloc, _, _ in res:
        U[gids] = Uloc
    rows = [r[3] for r in res]
    assert rows[0] == rows[1]
    row = rows[0]
    om = ost.build(OMesh(msh.coords, msh.cells))
    ref = dref.reference(om, U, window=(0.0, streamer.CHANNEL[1], 0.0, streamer.BOX), psi=msh.coords[:, 1] / streamer.BOX,
                         group=_electrodes(msh.coords), n_groups=2)
    for name, got, r, factor in (("N_i", row["N_i"], ref["species"][0], 1.0), ("N_e", row["N_e"], ref["species"][1], 1.0),
                                 ("cathode", row["surface_charge_cathode"], ref["groups"][0], epsilon_0),
                                 ("anode", row["surface_charge_anode"], ref["groups"][1], epsilon_0),
                                 ("current", row["current"], ref["current"], elementary_charge)):
        ratio = abs(got / factor - r.value) / r.abs
        print(f"[diagnostics] two ranks: {name} {ratio:.2e}", flush=True)
        assert ratio <= SUM_BOUND + 4 * EPS, name            # (4 eps: the row's multiplication by eps0 or e, undone here)
    assert abs(row["E_max"] - ref["field"].value) <= MAX_BOUND * ref["field"].value
    assert abs(row["E_max_axis"] - ref["window"].value) <= MAX_BOUND * ref["window"].value
    if ref["field"].unique:
        assert row["field_max_cell"] == ref["field"].index
    if ref["window"].unique:
        assert row["window_max_cell"] == ref["window"].index and row["z_head"] == ref["window"].centroid[1]
    assert row["ne_max"] == np.exp(ref["nodal"][1].value) and row["ni_max"] == np.exp(ref["nodal"][0].value)
    assert row["ni_max_vertex"] == ref["nodal"][0].index


# ---- 8: the facade and the example ------------------------------------------------------------------------------------------
def test_facade_and_example_rows(tmp_path):
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from fedm_amd import functions as ff
    from fedm_amd.physical_constants import elementary_charge, epsilon_0
    spec = importlib.util.spec_from_file_location("ex_streamer_diag", ROOT / "examples" / "streamer_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = types.SimpleNamespace(problem=None, states=[], direct=[])

    def build(J, F, bcs):
        """fedm.Problem, with the state downloaded whenever the example asks for a row"""
        p = ff.Problem(J, F, bcs)
        asked = p.device.diagnostics

        def recording(*a, **k):
            seen.states.append(p.device.get_state())
            d = asked(*a, **k)
            seen.direct.append(d)
            return d
        p.device.diagnostics = recording
        seen.problem = p
        return p
    out = tmp_path / "rows.txt"
    state, _ = mod.main(cells=24, end_time=1e-11, output_dir=tmp_path, quiet=True, stop_before_device=build,
                        diagnostics=out)
    rows = np.loadtxt(out).reshape(-1, len(mod.DIAGNOSTICS_COLUMNS))
    assert open(out).readline().split()[1:] == list(mod.DIAGNOSTICS_COLUMNS)
    assert rows.shape[0] == 2 == len(seen.states) and np.array_equal(seen.states[1], state)
    dev = seen.problem.device
    side = mod.Case().side
    window, psi = (0.0, mod.CHANNEL_RADIUS, 0.0, side), dev.coords[:, 1] / side
    group = _electrodes(dev.coords)
    # the facade's set-up is the device problem's: same groups, same numbers
    del dev.diagnostics                                  # (the recording wrapper)
    again = ff.Discharge_diagnostics(seen.problem, boundary_tags=(1, 2), window=window, weighting_potential=psi)()
    dev.diagnostics_setup(weighting_potential=psi, vertex_groups=group, n_groups=2)
    assert _bytes(again) == _bytes(dev.diagnostics(window=window)) == _bytes(seen.direct[1])
    om = ost.build(OMesh(dev.coords, dev.cells))
    times = [5e-12, 1e-11]
    for k, U in enumerate(seen.states):
        ref = dref.reference(om, U, window=window, psi=psi, group=group, n_groups=2)
        t, z_head, e_max, n_e, n_i, net, q_c, q_a, cur = rows[k]
        assert t == pytest.approx(times[k], rel=1e-12)
        for name, got, r, factor in (("N_e", n_e, ref["species"][1], 1.0), ("N_i", n_i, ref["species"][0], 1.0),
                                     ("cathode", q_c, ref["groups"][0], epsilon_0), ("anode", q_a, ref["groups"][1], epsilon_0),
                                     ("current", cur, ref["current"], elementary_charge)):
            ratio = abs(got / factor - r.value) / r.abs
            print(f"[diagnostics] example row {k}: {name} {ratio:.2e}", flush=True)
            assert ratio <= SUM_BOUND + 4 * EPS, (k, name)
        assert net == n_i - n_e
        assert abs(e_max - ref["window"].value) <= MAX_BOUND * ref["window"].value
        if ref["window"].unique:
            assert z_head == ref["window"].centroid[1]
