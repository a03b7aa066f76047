"""Electrode currents on the device (csrc/currents.hip, DeviceProblem.currents) against the numpy restatement of
tests/currents_reference.py, which tests/test_currents_reference.py pins on closed forms, against the two older device
quantities (Diagnostics.induced_current, Balance.induced_current), and against the device's own assembled residual.

LFA meshes, those of tests/test_gpu_diagnostics.py: (a) 3 x 3 -- 18 cells, less than one wave; (b) 12 x 17; (c) the graded
Delaunay mesh; (d) 182 x 182 -- 66 248 cells, more than CUR_BLOCKS x CUR_THREADS = 65 536, so the stride loop runs.  LFA
models: closed-form, planar, tabulated, the linear representation, the 'reaction' ion with coefficients, the four-species
model with a prescribed drift.  LMEA: the 18-cell, the 10 x 10 crossed and the irregular mesh with the models of
tests/lmea_models.py, NEQ 3 to 6, axisymmetric and planar.  States: tests/test_currents_reference.py's (three different
ones, dt != dt_old).  Potentials: n_psi = 1, 3 and 8 given ones (currents_reference.test_potentials: z/BOX + 0.2 (r/BOX)^2
scaled and shifted per slot, no two proportional), and the two solved ones of the box's electrodes.

Bounds.  Sums: |device - fsum| <= 1e-12 sum |terms| of the restatement (the bound of tests/test_gpu_diagnostics.py and
tests/test_gpu_balance.py).  The residual identity: 1e-11 sum |terms| (tests/test_gpu_balance.py's for its row identity).
The solve: |b - A psi|_2 <= 2 rtol |b|_2 on the free rows (the margin tests/test_gpu_gd_fields.py gives the consistent
projection's true residual over the recurrence's) and |psi - psi_direct|_2 <= |b - A psi|_2 / lambda_min(A).  Every figure is
printed before it is asserted.

A right-hand side that is not finite is refused (-2) like every argument that is not finite; FEDM_DIVERGED_NAN is shown with
an operator that is not positive definite.  Both leave the installed potentials as they were.
"""
import ctypes as C
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import currents_reference as cref  # noqa: E402
import tabulated_reference as tr  # noqa: E402
import test_currents_reference as tb  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SUM_BOUND, IDENTITY_BOUND, RTOL = 1e-12, 1e-11, 1e-10


class Lfa:
    """One (mesh, model) of the LFA family with its device problem; restatements are made once per potential set."""
    lmea = False

    def __init__(self, mesh_name, kind):
        self.c = c = tb.lfa_case(mesh_name, kind)
        self.prob = tr.device_streamer_problem(c.mesh.coords, c.mesh.cells, c.dm)
        self.reset()
        self._ref = {}

    def reset(self):
        self.prob.set_state(self.c.U, self.c.Uo, self.c.Uo1)
        self.prob.set_step(self.c.dt, self.c.dt_old)

    def potentials(self, n):
        return cref.test_potentials(self.c.mesh.coords, self.c.box, n, self.c.r0)

    def restate(self, psis, states=None):
        return tb.lfa_restate(self.c, psis, states=states)

    def ref(self, n):
        if n not in self._ref:
            self._ref[n] = self.restate(self.potentials(n))
        return self._ref[n]

    @property
    def charge_over_eps(self):
        from fedm_amd.physical_constants import elementary_charge, epsilon_0
        return elementary_charge / epsilon_0


class Lmea(Lfa):
    lmea = True

    def __init__(self, name, mesh_name, planar):
        from fedm_amd.device import DeviceProblem
        self.c = c = tb.lmea_case(name, mesh_name, planar)
        cc = c.c
        self.prob = DeviceProblem(c.mesh.coords, c.mesh.cells, c.model, facet_tags=c.mesh.tags,
                                  dirichlet_dofs=cc.dirichlet_dofs, dirichlet_vals=cc.dirichlet_vals, reorder=True)
        self.prob.set_gd_fields(c.fields)
        self.reset()
        self._ref = {}

    def restate(self, psis, states=None):
        return tb.lmea_restate(self.c, psis, states=states)

    @property
    def charge_over_eps(self):
        return float(self.c.md.charge_over_eps)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(*key):
        if key not in made:
            made[key] = Lfa(*key) if len(key) == 2 else Lmea(*key)
        return made[key]
    yield get
    for c in made.values():
        c.prob.close()


def _ratio(got, r):
    return abs(got - r.value) / r.abs if r.abs > 0.0 else (0.0 if got == 0.0 else math.inf)


def _check_sums(what, cur, ref):
    """Every sum of one call against the restatement; prints the worst ratio to sum |terms| per output first."""
    n = len(ref["conduction"])
    worst = {}
    for k in cref.OUTPUTS:
        worst[k] = max(_ratio(cur.raw[k][g], ref[k][g]) for g in range(n))
    worst["capacitance"] = max(_ratio(cur.raw["capacitance"][g, h], ref["capacitance"][g][h]) for g in range(n) for h in range(n))
    print(f"[currents] {what}, n_psi {n}: worst |device - fsum| / sum|terms| " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()),
          flush=True)
    assert cur.finite and cur.raw["conduction"].size == n and cur.raw["capacitance"].shape == (n, n)
    for k, v in worst.items():
        assert v <= SUM_BOUND, (what, k, v)
    assert np.array_equal(cur.raw["capacitance"], cur.raw["capacitance"].T)


def _bytes(cur):
    return b"".join(np.ascontiguousarray(cur.raw[k]).tobytes() for k in (*cref.OUTPUTS, "capacitance")) + bytes([cur.finite])


# ---- 1: the sums ------------------------------------------------------------------------------------------------------------
LFA_SUMS = [("a", "closed", 1), ("b", "closed", 3), ("c", "closed", 8), ("d", "closed", 3), ("b", "planar", 8), ("c", "planar", 1),
            ("a", "tabulated", 3), ("c", "tabulated", 8), ("d", "tabulated", 1), ("b", "linear", 3), ("b", "reaction", 8)]
LMEA_SUMS = [("e-only", "3x3", False, 1), ("e-only", "10x10", True, 3), ("ion-e", "10x10", False, 8), ("ion-e", "3x3", False, 3),
             ("deck-shape-permuted", "irregular", False, 3), ("deck-shape-permuted", "10x10", False, 1),
             ("two-ions-small", "10x10", True, 8), ("two-ions-small", "3x3", False, 1), ("two-ions-full", "irregular", False, 8),
             ("two-ions-full", "10x10", False, 3)]


def _sums(c, what, n_psi):
    c.reset()
    c.prob.currents_setup(potentials=c.potentials(n_psi))
    cur = c.prob.currents()
    _check_sums(what, cur, c.ref(n_psi))
    from fedm_amd.physical_constants import elementary_charge, epsilon_0
    assert np.array_equal(cur.conduction, elementary_charge * cur.raw["conduction"])
    assert np.array_equal(cur.displacement, epsilon_0 * cur.raw["displacement"])
    assert np.array_equal(cur.total, cur.conduction + cur.displacement)
    assert np.array_equal(cur.capacitance, epsilon_0 * cur.raw["capacitance"])
    assert np.array_equal(cur.induced_charge, elementary_charge * cur.raw["induced_charge"])
    assert np.array_equal(c.prob.currents_psi(), c.potentials(n_psi))
    return cur


@pytest.mark.parametrize("mesh_name,kind,n_psi", LFA_SUMS)
def test_lfa_sums_against_the_restatement(cases, mesh_name, kind, n_psi):
    c = cases(mesh_name, kind)
    if mesh_name == "d":
        assert c.c.mesh.nc == 66248 > 256 * 256
    _sums(c, f"LFA mesh ({mesh_name}) {kind}", n_psi)


@pytest.mark.parametrize("name,mesh_name,planar,n_psi", LMEA_SUMS)
def test_lmea_sums_against_the_restatement(cases, name, mesh_name, planar, n_psi):
    c = cases(name, mesh_name, planar)
    assert c.prob.n_eq == {"e-only": 3, "ion-e": 4, "deck-shape-permuted": 5}.get(name, 6)
    _sums(c, f"LMEA {name} {mesh_name} {'planar' if planar else 'axisymmetric'}", n_psi)


def test_four_species_with_a_prescribed_drift():
    import lfa_models
    from oracle import streamer as ost
    import photoionization_reference as pr
    m, prob, om, _, _ = lfa_models.four_species_problem()
    try:
        U2 = pr.perturbed(ost.initial_state(ost.build(om.mesh)), 22)
        r, z = m.coords[:, 0], m.coords[:, 1]
        rng = np.random.default_rng(31)
        bump = np.exp(-(r ** 2 + (z - 0.008) ** 2) / (2e-3) ** 2)
        U = np.column_stack([np.log(1e12 + 1e15 * bump) + rng.normal(0, 0.2, r.size), U2[:, 0],
                             np.log(1e11 + 1e14 * bump) + rng.normal(0, 0.2, r.size), U2[:, 1], U2[:, 2]])
        Uo, Uo1 = tb._older(U, 47, 4)
        psis = cref.test_potentials(m.coords, ost.BOX, 3)
        prob.set_state(U, Uo, Uo1)
        prob.set_step(tb.LFA_DT, tb.LFA_DT_OLD)
        prob.currents_setup(potentials=psis)
        ref = cref.lfa_reference(om, U, Uo, Uo1, tb.LFA_DT, tb.LFA_DT_OLD, psis)
        cur = prob.currents()
        _check_sums("LFA four species", cur, ref)
        prob.diagnostics_setup(weighting_potential=psis[0])
        d = prob.diagnostics()
        assert abs(cur.raw["conduction"][0] - d.induced_current) <= SUM_BOUND * ref["conduction"][0].abs
    finally:
        prob.close()


# ---- 2: one potential: the older quantities ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("b", "closed"), ("c", "tabulated"), ("b", "linear"), ("b", "planar"),
                                 ("ion-e", "10x10", False), ("two-ions-full", "irregular", False), ("two-ions-small", "10x10", True)])
def test_conduction_is_the_older_induced_current(cases, key):
    c = cases(*key)
    c.reset()
    psi = c.potentials(1)
    c.prob.currents_setup(potentials=psi)
    cur = c.prob.currents()
    if c.lmea:
        c.prob.balance_setup(weighting_potential=psi[0])
        old = c.prob.balance()
    else:
        c.prob.diagnostics_setup(weighting_potential=psi[0])
        old = c.prob.diagnostics()
    ref = c.ref(1)["conduction"][0]
    ratio = abs(cur.raw["conduction"][0] - old.induced_current) / ref.abs
    print(f"[currents] {key}: conduction {cur.raw['conduction'][0]!r} induced_current {old.induced_current!r} "
          f"|difference| / sum|terms| {ratio:.2e}", flush=True)
    assert old.induced_current != 0.0 and ratio <= SUM_BOUND


# ---- the solved potentials ------------------------------------------------------------------------------------------------
def _solve(c, **kw):
    c.reset()
    its = c.prob.currents_setup(boundary_tags=(1, 2), rtol=RTOL, **kw)
    return its, c.prob.currents_psi()


def _groups(c):
    from fedm_amd.device import boundary_vertex_groups
    p = c.prob
    return boundary_vertex_groups(p.cells, p.facet_tags(), p.nv, p.dirichlet_vertices(), (1, 2))


# ---- 3: the Poisson rows tie coupling, induced charge and the electrodes' row sums together ---------------------------------
@pytest.mark.parametrize("key", [("b", "closed"), ("c", "tabulated"), ("b", "planar"), ("ion-e", "10x10", False),
                                 ("two-ions-small", "10x10", True), ("deck-shape-permuted", "irregular", False)])
def test_identity_with_the_assembled_poisson_rows(cases, key):
    c = cases(*key)
    _, psi = _solve(c)
    group = _groups(c)
    cur = c.prob.currents()
    if c.lmea:
        c.prob.balance_setup(vertex_groups=group, n_groups=2)
        gs = c.prob.balance().group_sum
    else:
        c.prob.diagnostics_setup(vertex_groups=group, n_groups=2)
        gs = c.prob.diagnostics().group_sum
    F, _ = c.prob.residual()
    Fphi = F.reshape(c.prob.nv, c.prob.n_eq)[:, -1]
    free = np.ones(c.prob.nv, dtype=bool)
    free[c.prob.dirichlet_vertices()] = False
    ref = c.restate(psi)
    coe = c.charge_over_eps
    for g in range(2):
        lhs = cur.raw["coupling"][g] - coe * cur.raw["induced_charge"][g]
        rhs = gs[g] + math.fsum((psi[g][free] * Fphi[free]).tolist())
        scale = ref["coupling"][g].abs + coe * ref["induced_charge"][g].abs
        ratio = abs(lhs - rhs) / scale
        print(f"[currents] {key} electrode {g}: coupling - (e/eps0) charge {lhs:.9e}, group sum + psi . F {rhs:.9e}, "
              f"|difference| / sum|terms| {ratio:.2e}", flush=True)
        assert ratio <= IDENTITY_BOUND, (key, g, ratio)
        assert abs(lhs) >= 1e-6 * scale


# ---- 4: displacement = capacitance x D_t V, whatever the potentials -------------------------------------------------------
@pytest.mark.parametrize("key", [("b", "closed"), ("a", "tabulated"), ("c", "planar"), ("e-only", "3x3", False),
                                 ("two-ions-full", "10x10", False)])
def test_displacement_is_capacitance_times_the_rate_of_the_voltages(cases, key):
    c = cases(*key)
    c.reset()
    psis = c.potentials(3)
    c.prob.currents_setup(potentials=psis)
    V = np.array([[-250.0, 120.0, 35.0], [-180.0, 150.0, -20.0], [-75.0, 90.0, 5.0]])       # V_h at t_new, t_old, t_old1
    iphi = c.prob.n_eq - 1
    states = []
    for k, S in enumerate((c.c.U, c.c.Uo, c.c.Uo1)):
        S = S.copy()
        S[:, iphi] = V[k] @ psis
        states.append(S)
    try:
        c.prob.set_state(*states)
        cur = c.prob.currents()
    finally:
        c.reset()
    ref = c.restate(psis, states=tuple(states))
    DtV = cref.bdf2_weights(c.c.dt, c.c.dt_old) @ V
    cap = cur.raw["capacitance"]
    for g in range(3):
        want = math.fsum((cap[g] * DtV).tolist())
        scale = ref["displacement"][g].abs + sum(abs(DtV[h]) * ref["capacitance"][g][h].abs for h in range(3))
        ratio = abs(cur.raw["displacement"][g] - want) / scale
        print(f"[currents] {key}: displacement[{g}] {cur.raw['displacement'][g]:.9e}, sum_h C[g][h] D_tV_h {want:.9e}, "
              f"|difference| / sum|terms| {ratio:.2e}", flush=True)
        assert ratio <= SUM_BOUND, (key, g, ratio)
        assert abs(want) >= 1e-6 * scale


# ---- 5: the two electrodes' potentials add up to 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("b", "closed"), ("c", "closed"), ("ion-e", "10x10", False), ("two-ions-small", "10x10", True)])
def test_the_two_solved_potentials_sum_to_one(cases, key):
    c = cases(*key)
    _, psi = _solve(c)
    delta = float(np.abs(psi[0] + psi[1] - 1.0).max())
    cur = c.prob.currents()
    ref = c.restate(psi)
    _check_sums(f"{key} solved", cur, ref)
    print(f"[currents] {key}: max |psi_0 + psi_1 - 1| {delta:.2e}", flush=True)
    assert delta <= 1e-6
    rows = [("conduction", cur.raw["conduction"], ref["conduction"]), ("displacement", cur.raw["displacement"], ref["displacement"])]
    rows += [(f"capacitance[{g}]", cur.raw["capacitance"][g], ref["capacitance"][g]) for g in range(2)]
    for name, got, r in rows:
        total, scale = got[0] + got[1], r[0].abs + r[1].abs
        print(f"[currents] {key}: {name} sums to {total:.3e}, bound {(delta + SUM_BOUND) * scale:.3e}", flush=True)
        assert abs(total) <= (delta + SUM_BOUND) * scale, (key, name)


# ---- 6: the solve -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("a", "closed"), ("b", "closed"), ("c", "closed"), ("e-only", "3x3", False),
                                 ("ion-e", "10x10", False), ("deck-shape-permuted", "irregular", False)])
@pytest.mark.parametrize("multigrid", [False, True])
def test_the_solve(cases, key, multigrid):
    """MEASURED on the MI355X at rtol = 1e-10: |b - A psi|_2 / (rtol |b|_2) 0.40 .. 0.92 (Jacobi: 63 to 117 CG steps on the
    234- to 717-vertex meshes; with the hierarchy 14 to 17), below 1e-3 where CG ends exactly (8 free vertices, 8 steps;
    the crossed 10 x 10 mesh under Jacobi, 19 steps); |psi - psi_direct|_2 lambda_min / |b - A psi|_2 0.012 .. 0.27."""
    c = cases(*key)
    its, psi = _solve(c, multigrid=multigrid, max_coarse=12)
    levels, rhs, fixed = c.prob.currents_system
    A = levels[0][0]
    if multigrid and c.prob.nv > 100:
        assert len(levels) >= 2, c.prob.currents_levels
    assert len(levels) == (len(c.prob.currents_levels)) and (multigrid or len(levels) == 1)
    group = _groups(c)
    order = c.prob._order
    Ad = A.toarray()
    Aff = Ad[np.ix_(~fixed, ~fixed)]
    lam = float(np.linalg.eigvalsh(Aff)[0])
    assert lam > 0.0
    for g in range(2):
        p = psi[g][order]                                    # the device's numbering
        assert np.array_equal(psi[g][group == g + 1], np.ones((group == g + 1).sum()))          # bitwise
        others = np.zeros(c.prob.nv, dtype=bool)
        others[c.prob.dirichlet_vertices()] = True
        others &= group != g + 1
        assert np.array_equal(psi[g][others], np.zeros(others.sum())) and others.any()
        b = rhs[g][~fixed]
        resid = float(np.linalg.norm(b - Aff @ p[~fixed]))
        bnorm = float(np.linalg.norm(b))
        dist = float(np.linalg.norm(p[~fixed] - np.linalg.solve(Aff, b)))
        print(f"[currents] {key} multigrid={multigrid} levels {c.prob.currents_levels} electrode {g}: {its[g]} iterations, "
              f"|b - A psi| / (rtol |b|) {resid / (RTOL * bnorm):.3f}, |psi - psi_direct| lambda_min / |b - A psi| "
              f"{dist * lam / resid if resid > 0 else 0.0:.3f}", flush=True)
        assert its[g] > 0 and bnorm > 0.0
        assert resid <= 2 * RTOL * bnorm, (key, g)
        assert dist <= resid / lam, (key, g)


def test_a_failed_solve_leaves_the_potentials(cases):
    c = cases("b", "closed")
    _, psi = _solve(c)
    first = c.prob.currents()
    levels, rhs, fixed = c.prob.currents_system
    A = levels[0][0]
    bad = rhs.copy()
    bad[1, np.nonzero(~fixed)[0][3]] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        c.prob.currents_solve([(A, None)], bad, RTOL)
    assert np.array_equal(c.prob.currents_psi(), psi)
    with pytest.raises(RuntimeError, match="positive definite"):              # FEDM_DIVERGED_NAN
        c.prob.currents_solve([(-A, None)], rhs, RTOL)
    assert np.array_equal(c.prob.currents_psi(), psi)
    start = psi.copy()
    start[:, c.prob._order[np.nonzero(~fixed)[0]]] = 0.5
    c.prob.currents_setup(potentials=start)
    with pytest.raises(RuntimeError, match="max_it = 1"):                     # FEDM_DIVERGED_LINEAR
        c.prob.currents_solve([(A, None)], rhs, RTOL, max_it=1)
    assert np.array_equal(c.prob.currents_psi(), start)
    assert c.prob.currents_solve([(A, None)], rhs, RTOL) and np.abs(c.prob.currents_psi() - psi).max() <= 1e-7
    c.prob.currents_setup(potentials=psi)
    assert _bytes(c.prob.currents()) == _bytes(first)


# ---- 7: invariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("d", "closed"), ("two-ions-full", "irregular", False)])
def test_two_calls_agree_byte_for_byte_and_nothing_is_touched(cases, key):
    c = cases(*key)
    c.reset()
    c.prob.currents_setup(potentials=c.potentials(8))
    if not c.lmea:      # the LDS patches add with atomics; the global colouring is the bitwise reproducible LFA assembly
        c.prob.set_assembly("colour")
    try:
        F0, _ = c.prob.residual()
        U0 = c.prob.get_state()
        f0 = c.prob.get_gd_fields() if c.lmea else None
        first = c.prob.currents()
        assert _bytes(c.prob.currents()) == _bytes(first)
        assert np.array_equal(c.prob.get_state(), U0) and np.array_equal(c.prob.get_state_old(), c.c.Uo)
        if c.lmea:
            assert np.array_equal(c.prob.get_gd_fields(), f0)
        F1, _ = c.prob.residual()
        assert np.array_equal(F1, F0)
        assert _bytes(c.prob.currents()) == _bytes(first)
    finally:
        if not c.lmea:
            c.prob.set_assembly("patch")


@pytest.mark.parametrize("key", [("b", "closed"), ("ion-e", "10x10", False)])
def test_a_nan_in_the_potential_is_flagged_and_the_next_call_is_clean(cases, key):
    c = cases(*key)
    c.reset()
    c.prob.currents_setup(potentials=c.potentials(3))
    first = c.prob.currents()
    iphi = c.prob.n_eq - 1
    try:
        for which, value in (("u_new", np.nan), ("u_new", np.inf), ("u_old", np.nan)):
            bad = (c.c.U if which == "u_new" else c.c.Uo).copy()
            bad[c.prob.nv // 2, iphi] = value
            c.prob.set_state(**{which: bad})
            assert c.prob.currents().finite is False, (which, value)
            c.reset()
    finally:
        c.reset()
    again = c.prob.currents()
    assert again.finite is True and _bytes(again) == _bytes(first)


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(cases):
    from fedm_amd import _lib
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum
    for key in (("b", "closed"), ("ion-e", "10x10", False)):
        c = cases(*key)
        c.reset()
        lib, h, nv = c.prob.lib, c.prob._h, c.prob.nv
        good = c.potentials(2)
        c.prob.currents_setup(potentials=good)
        psi9 = np.zeros((9, nv))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))          # noqa: E731
        out = _lib.CurrentsOut()
        assert lib.fedm_currents_setup(h, 0, dp(psi9)) == -2 and "0 weighting potentials" in _lib.last_error()
        assert lib.fedm_currents_setup(h, 9, dp(psi9)) == -2 and "9 weighting potentials" in _lib.last_error()
        assert lib.fedm_currents_setup(h, 1, None) == -2 and "null" in _lib.last_error()
        psi9[1, 7] = np.inf
        assert lib.fedm_currents_setup(h, 2, dp(psi9)) == -2 and "psi[1][7]" in _lib.last_error()
        assert lib.fedm_currents(h, None) == -2 and "null" in _lib.last_error()
        assert lib.fedm_currents_get_psi(h, None) == -2 and "null" in _lib.last_error()
        rhs = np.zeros((2, nv))
        assert lib.fedm_currents_solve(h, None, dp(rhs), 1e-10, 10, None) == -2 and "null" in _lib.last_error()
        hier = _lib.PhotoHierarchy()
        assert lib.fedm_currents_solve(h, C.byref(hier), None, 1e-10, 10, None) == -2 and "null" in _lib.last_error()
        assert lib.fedm_currents_solve(h, C.byref(hier), dp(rhs), 1e-10, 10, None) == -2 and "hierarchy" in _lib.last_error()
        from fedm_amd import amg
        import scipy.sparse as sp
        keep = []
        eye = amg._csr_struct(sp.identity(nv, format="csr"), keep)
        small = amg._csr_struct(sp.identity(nv - 1, format="csr"), keep)
        hier.n_levels, hier.nu, hier.A = 2, 1, C.pointer(eye)
        assert lib.fedm_currents_solve(h, C.byref(hier), dp(rhs), 1e-10, 10, None) == -2 and "hierarchy" in _lib.last_error()
        hier.n_levels, hier.A = 1, C.pointer(small)
        assert lib.fedm_currents_solve(h, C.byref(hier), dp(rhs), 1e-10, 10, None) == -2 and "rows" in _lib.last_error()
        hier.A = C.pointer(eye)
        assert lib.fedm_currents_solve(h, C.byref(hier), dp(rhs), 0.0, 10, None) == -2 and "rtol" in _lib.last_error()
        assert lib.fedm_currents_solve(h, C.byref(hier), dp(rhs), 1e-10, -1, None) == -2 and "max_it" in _lib.last_error()
        rhs[0, 3] = np.nan
        assert lib.fedm_currents_solve(h, C.byref(hier), dp(rhs), 1e-10, 10, None) == -2 and "rhs[0][3]" in _lib.last_error()
        # every refusal left the set-up in place
        assert np.array_equal(c.prob.currents_psi(), good) and c.prob.currents().finite
        with pytest.raises(ValueError, match="either"):
            c.prob.currents_setup()
        with pytest.raises(ValueError, match="1 to 8"):
            c.prob.currents_setup(potentials=np.zeros((9, nv)))
    # before a set-up
    m = streamer.mesh(4)
    fresh = streamer.device_problem(m.coords, m.cells)
    try:
        out = _lib.CurrentsOut()
        rhs = np.zeros((1, fresh.nv))
        hier = _lib.PhotoHierarchy()
        assert fresh.lib.fedm_currents(fresh._h, C.byref(out)) == -2 and "fedm_currents_setup has not" in _lib.last_error()
        assert fresh.lib.fedm_currents_solve(fresh._h, C.byref(hier), dp(rhs), 1e-10, 10, None) == -2
        assert "fedm_currents_setup has not" in _lib.last_error()
        assert fresh.lib.fedm_currents_get_psi(fresh._h, dp(rhs)) == -2 and "fedm_currents_setup has not" in _lib.last_error()
        with pytest.raises(RuntimeError, match="has not been called"):
            fresh.currents()
    finally:
        fresh.close()
    # no Poisson equation
    msh = Mesh(m.coords, m.cells)
    dm = Model(n_species=1, poisson=False, eq_type=["diffusion-reaction"], Z=[-1.0], D=[TermSum.const(0.1)],
               reactions=[Reaction(TermSum.const(1.0), power=[1], net=[1])], bc_kind=[["zero flux"]] * 4, quadrature_degree=2)
    plain = DeviceProblem(msh.coords, msh.cells, dm, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES))
    try:
        psi = np.zeros((1, plain.nv))
        assert plain.lib.fedm_currents_setup(plain._h, 1, dp(psi)) == -2 and "Poisson" in _lib.last_error()
        assert plain.lib.fedm_currents(plain._h, C.byref(out)) == -2 and "Poisson" in _lib.last_error()
        with pytest.raises(RuntimeError, match="Poisson"):
            plain.currents_setup(boundary_tags=(1, 2))
    finally:
        plain.close()


def test_a_context_with_ghosts_is_refused(cases):
    from fedm_amd import _lib
    from fedm_amd.device import DeviceProblem
    c = cases("ion-e", "10x10", False)
    cc = c.c.c
    prob = DeviceProblem(c.c.mesh.coords, c.c.mesh.cells, c.c.model, facet_tags=c.c.mesh.tags, dirichlet_dofs=cc.dirichlet_dofs,
                         dirichlet_vals=cc.dirichlet_vals, n_owned=c.c.mesh.nv - 3)
    try:
        psi = np.zeros((1, prob.nv))
        out = _lib.CurrentsOut()
        assert prob.lib.fedm_currents_setup(prob._h, 1, psi.ctypes.data_as(C.POINTER(C.c_double))) == -2
        assert "ghost" in _lib.last_error()
        assert prob.lib.fedm_currents(prob._h, C.byref(out)) == -2 and "ghost" in _lib.last_error()
    finally:
        prob.close()


@pytest.mark.parametrize("key", [("b", "closed"), ("ion-e", "10x10", False)])
def test_a_refused_setup_leaves_the_count_with_the_potentials(cases, key):
    """Three potentials installed, then every way a set-up is refused: currents_psi() still returns the three (the
    library writes as many rows as IT holds), and a call still gives three currents."""
    c = cases(*key)
    c.reset()
    good = c.potentials(3)
    c.prob.currents_setup(potentials=good)
    first = c.prob.currents()
    bad = good.copy()
    bad[2, 5] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        c.prob.currents_setup(potentials=bad)
    assert np.array_equal(c.prob.currents_psi(), good)
    with pytest.raises(ValueError, match="1 to 8"):
        c.prob.currents_setup(potentials=np.zeros((9, c.prob.nv)))
    assert np.array_equal(c.prob.currents_psi(), good)
    with pytest.raises(ValueError, match="either"):
        c.prob.currents_setup()
    with pytest.raises(ValueError, match="belongs to one group"):
        c.prob.currents_setup(boundary_tags=(1, 1))
    with pytest.raises(ValueError):
        c.prob.currents_setup(potentials=np.zeros((2, c.prob.nv + 1)))
    psi = c.prob.currents_psi()
    assert psi.shape == (3, c.prob.nv) and np.array_equal(psi, good)
    assert _bytes(c.prob.currents()) == _bytes(first) and first.raw["conduction"].size == 3
    # a failed solve keeps the count too
    import scipy.sparse as sp
    levels, rhs = [(-sp.identity(c.prob.nv, format="csr"), None)], np.ones((3, c.prob.nv))
    with pytest.raises(RuntimeError, match="positive definite"):
        c.prob.currents_solve(levels, rhs, RTOL)
    assert len(c.prob.last_currents_iterations) == 3 and np.array_equal(c.prob.currents_psi(), good)


def test_a_vertex_in_two_electrodes_is_a_value_error(cases):
    c = cases("b", "closed")
    with pytest.raises(ValueError, match="belongs to one group"):
        c.prob.currents_setup(boundary_tags=(1, 1))


# ---- 9: the facade, the cases and the examples ----------------------------------------------------------------------------
def test_electrode_currents_is_the_device_problems(cases):
    from fedm_amd import functions as ff
    for key in (("b", "closed"), ("ion-e", "10x10", False)):
        c = cases(*key)
        c.reset()
        call = ff.Electrode_currents(c.prob, boundary_tags=(1, 2), rtol=RTOL)
        assert _bytes(call()) == _bytes(c.prob.currents()) and np.array_equal(call.psi, c.prob.currents_psi())
        assert len(call.iterations) == 2 and min(call.iterations) > 0
        given = ff.Electrode_currents(c.prob, weighting_potentials=c.potentials(3))
        assert _bytes(given()) == _bytes(c.prob.currents()) and np.array_equal(given.psi, c.potentials(3))
        assert given().raw["conduction"].size == 3 and given.iterations == []


def _example(name):
    spec = importlib.util.spec_from_file_location(f"{name}_example_currents", ROOT / "examples" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _recording(seen):
    from fedm_amd import functions as ff

    def build(J, F, bcs):
        p = ff.Problem(J, F, bcs)
        asked = p.device.currents

        def recording():
            cur = asked()
            seen["currents"].append(cur)
            return cur
        p.device.currents = recording
        seen["problem"] = p
        return p
    return build


def _rows_are_the_device_values(rows, seen, mod):
    assert rows.shape == (len(seen["currents"]), len(mod.CURRENTS_COLUMNS)) and rows.shape[0] >= 2
    for k, cur in enumerate(seen["currents"]):
        want = [cur.conduction[0], cur.displacement[0], cur.total[0], cur.conduction[1], cur.displacement[1], cur.total[1]]
        assert np.array_equal(rows[k, 1:], np.array(want)), k
        assert cur.finite and cur.conduction[0] != 0.0


def test_glow_example_rows_are_the_device_values(tmp_path):
    mod = _example("glow_discharge")
    seen = dict(problem=None, currents=[])
    out = tmp_path / "currents.txt"
    res = mod.main(nx=8, ny=8, T_final=2e-13, output_dir=tmp_path / "run", stop_before_device=_recording(seen), currents=out)
    rows = np.atleast_2d(np.loadtxt(out))
    assert res["steps"] == rows.shape[0]
    _rows_are_the_device_values(rows, seen, mod)
    # the powered electrode's voltage rises: a displacement current flows, and what leaves one electrode enters the other
    last = seen["currents"][-1]
    assert last.displacement[0] != 0.0
    assert abs(last.total[0] + last.total[1]) <= 1e-6 * (abs(last.total[0]) + abs(last.total[1]))


def test_streamer_example_rows_are_the_device_values(tmp_path):
    mod = _example("streamer_discharge")
    seen = dict(problem=None, currents=[])
    out = tmp_path / "currents.txt"
    mod.main(cells=12, end_time=1e-11, output_dir=tmp_path / "run", quiet=True, stop_before_device=_recording(seen), currents=out)
    rows = np.atleast_2d(np.loadtxt(out))
    _rows_are_the_device_values(rows, seen, mod)


def test_stepper_currents_is_the_facade():
    from fedm_amd.cases import streamer
    m = streamer.mesh(12)
    prob = streamer.device_problem(m.coords, m.cells)
    try:
        st = streamer.Stepper(prob)
        st.initialise()
        st.step()
        st.step()
        cur = st.currents()
        assert cur.finite and _bytes(cur) == _bytes(prob.currents()) and cur.conduction.size == 2
        psi = prob.currents_psi()
        assert np.abs(psi[0] + psi[1] - 1.0).max() <= 1e-8
    finally:
        prob.close()


# ---- 10: keep_currents takes the currents of the residual just solved ---------------------------------------------------------
def test_keep_currents_is_taken_between_the_solve_and_the_mean_energy_refresh():
    """MEASURED on the MI355X (6 x 6 mesh, two steps): the call after ``step()`` returns the kept conduction bit for bit,
    -5.41039254e+11 / 5.41039254e+11 per second -- unlike the balance, whose wall terms read the mean-energy row that the
    refresh rewrites, the fluxes read the rows gd_prep_step writes (mu, D, their derivatives, the old mean energy and the old
    electron density) -- and differs from it once the next step's shift and refresh have run."""
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=6, ny=6, T_final=1.0, keep_currents=True)
    try:
        assert case.device_pipeline and case.last_currents is None
        case.step()
        order = []
        prob = case.prob
        asked, refresh, solve = prob.currents, prob.gd_update_mean_energy, prob.newton_solve

        def currents():
            order.append("currents")
            order.append(asked())
            return order[-1]

        def update():
            order.append("refresh")
            return refresh()

        def newton(*a, **kw):
            order.append("solve")
            return solve(*a, **kw)
        prob.currents, prob.gd_update_mean_energy, prob.newton_solve = currents, update, newton
        try:
            case.step()
        finally:
            del prob.currents, prob.gd_update_mean_energy, prob.newton_solve
        names = [o for o in order if isinstance(o, str)]
        assert names[-2:] == ["currents", "refresh"] and "solve" in names[:-2], names
        kept = case.last_currents
        assert kept is order[-2] and kept.finite
        after = case.currents()
        print(f"[currents] keep_currents: conduction kept {kept.raw['conduction']!r}, after step() {after.raw['conduction']!r}",
              flush=True)
        # nothing the currents read has moved: the same bytes
        assert _bytes(after) == _bytes(kept)
        plain = gdc.Case(nx=6, ny=6, T_final=1.0)
        try:
            plain.step()
            plain.step()
            assert plain.last_currents is None and plain.t == case.t
            assert _bytes(plain.currents()) == _bytes(kept)
        finally:
            plain.prob.close()
        # the beginning of the next step: the states shift and the table moves on, and so do the currents
        prob.shift_state()
        prob.gd_prep_step()
        later = prob.currents()
        print(f"[currents] keep_currents: conduction after the next step's refresh {later.raw['conduction']!r}", flush=True)
        assert later.finite and np.all(later.raw["conduction"] != kept.raw["conduction"])
        assert np.array_equal(later.raw["capacitance"], kept.raw["capacitance"])
    finally:
        case.prob.close()
