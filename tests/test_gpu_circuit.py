"""The external circuit on the device (csrc/circuit.hip, DeviceProblem.circuit_*, fedm.External_circuit) against the numpy
restatement of tests/circuit_reference.py, which tests/test_circuit_reference.py pins on closed forms.

Meshes: the 18-cell mesh and the 10 x 10 crossed mesh of the currents tests (the four-species model on its own 20 x 20).
Bounds.  Conduction and conductance: |device - fsum| <= 1e-12 sum |terms| of the restatement, the bound of
tests/test_gpu_currents.py.  The advance: |U - U_restated| <= 1e-13 of the case's largest voltage, from the device's own
measured quantities and history (both eliminate an at most 3 x 3 system with partial pivoting in doubles; the systems'
condition numbers are printed); dU/dt and the lead current to 1e-13 of the sum of the magnitudes of their terms.  The
vacuum run: U to 1e-12 of the source's voltage over 20 steps, Kirchhoff's closure against the displacement form of
fedm_currents to 100 x the Newton tolerance 1e-10.  The plasma run: states and U to 1e-9 of each component's largest value,
the bound of tests/test_gpu_parity.py for a Newton step solved to 1e-8 on both sides.  Every figure is printed before it
is asserted.
"""
import ctypes as C
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import circuit_reference as circ  # noqa: E402
import currents_reference as cref  # noqa: E402
import tabulated_reference as tr  # noqa: E402
import test_circuit_reference as tc  # noqa: E402
import test_currents_reference as tb  # noqa: E402
import test_gpu_currents as tgc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SUM_BOUND, ADVANCE_BOUND, PARITY_BOUND = tc.SUM_BOUND, tc.ADVANCE_BOUND, 1e-9
NEWTON_RTOL, CLOSURE_BOUND = 1e-10, 100 * 1e-10


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(*key):
        if key not in made:
            made[key] = tgc.Lfa(*key) if len(key) == 2 else tgc.Lmea(*key)
        return made[key]
    yield get
    for c in made.values():
        c.prob.close()


def _no_entries(prob):
    return np.full(prob._ddofs.size, -1, dtype=np.int8)


def _bytes(s):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (s.raw["conduction"], s.raw["conductance"], s.U, s.U_old,
                                                                s.U_old1, s.dUdt, s.lead_current)) + bytes([s.flag])


def _check_measure(what, s, cond_ref, G_ref):
    n = len(cond_ref)
    worst_c = max(tgc._ratio(s.raw["conduction"][g], cond_ref[g]) for g in range(n))
    worst_g = max(tgc._ratio(s.raw["conductance"][g, h], G_ref[g][h]) for g in range(n) for h in range(n))
    print(f"[circuit] {what}, n {n}: worst |device - fsum| / sum|terms| conduction {worst_c:.2e} conductance {worst_g:.2e}",
          flush=True)
    assert s.flag == 0 and s.raw["conductance"].shape == (n, n)
    assert worst_c <= SUM_BOUND and worst_g <= SUM_BOUND, (what, worst_c, worst_g)
    assert np.array_equal(s.raw["conductance"], s.raw["conductance"].T)


def _measure(prob, psis=None, tags=None, R=1.0e3):
    if psis is not None:
        prob.currents_setup(potentials=psis)
        prob.circuit_setup(R, electrode_of_entry=_no_entries(prob))
    else:
        prob.currents_setup(boundary_tags=tags, rtol=tgc.RTOL)
        prob.circuit_setup(R, boundary_tags=tags)
    prob.circuit_measure()
    return prob.circuit_get()


# ---- 1: conduction and conductance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_psi", [("closed", 3), ("linear", 8), ("tabulated", 1)])
def test_lfa_measure_against_the_restatement(cases, kind, n_psi):
    c = cases("a", kind)
    c.reset()
    psis = c.potentials(n_psi)
    s = _measure(c.prob, psis)
    G = circ.lfa_conductance(c.c.om, c.c.U, psis)
    _check_measure(f"LFA 18 cells {kind}", s, c.ref(n_psi)["conduction"], G)
    assert all(G[g][g].value > 0.0 for g in range(n_psi))
    again = c.prob.circuit_get()
    c.prob.circuit_measure()                      # (the history moves, nothing else: U = U_old = U_old1 here)
    assert _bytes(c.prob.circuit_get()) == _bytes(again) == _bytes(s)


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
        s = _measure(prob, psis)
        ref = cref.lfa_reference(om, U, Uo, Uo1, tb.LFA_DT, tb.LFA_DT_OLD, psis)
        _check_measure("LFA four species, one with a prescribed drift", s, ref["conduction"], circ.lfa_conductance(om, U, psis))
    finally:
        prob.close()


@pytest.mark.parametrize("name,mesh_name,planar,n_psi", [("two-ions-full", "10x10", False, 3), ("ion-e", "3x3", False, 8)])
def test_lmea_measure_against_the_restatement(cases, name, mesh_name, planar, n_psi):
    c = cases(name, mesh_name, planar)
    c.reset()
    psis = c.potentials(n_psi)
    s = _measure(c.prob, psis)
    m = c.c
    G = circ.lmea_conductance(m.md, m.mesh.coords, m.mesh.cells, m.fields, m.U, m.c.rules[0], psis)
    _check_measure(f"LMEA {name} {mesh_name}", s, c.ref(n_psi)["conduction"], G)
    assert all(G[g][g].value > 0.0 for g in range(n_psi))
    c.prob.circuit_measure()
    assert _bytes(c.prob.circuit_get()) == _bytes(s)


def test_the_argon_deck_against_the_restatement():
    import lmea_models as lm
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=10, ny=10, T_final=1.0)
    try:
        case.step()
        case.step()
        prob = case.prob
        psis = cref.test_potentials(prob.coords, case.gap, 2)
        s = _measure(prob, psis)
        U, Uo, fields, md = prob.get_state(), prob.get_state_old(), prob.get_gd_fields(), prob.model.to_c()
        qp = lm.rules(4)[0]
        ref = cref.lmea_reference(md, prob.coords, prob.cells, fields, U, Uo, Uo, case.dt_old.time_step, 1e30, qp, psis)
        G = circ.lmea_conductance(md, prob.coords, prob.cells, fields, U, qp, psis)
        _check_measure("LMEA argon deck 10 x 10", s, ref["conduction"], G)
        assert G[0][0].value > 0.0
    finally:
        case.prob.close()


@pytest.mark.parametrize("key", [("a", "closed"), ("ion-e", "10x10", False)])
def test_two_solved_potentials(cases, key):
    c = cases(*key)
    c.reset()
    s = _measure(c.prob, tags=(1, 2))
    psi = c.prob.currents_psi()
    m = c.c
    G = (circ.lmea_conductance(m.md, m.mesh.coords, m.mesh.cells, m.fields, m.U, m.c.rules[0], psi) if c.lmea
         else circ.lfa_conductance(m.om, m.U, psi))
    _check_measure(f"{key} solved", s, c.restate(psi)["conduction"], G)
    c.prob.circuit_measure()
    assert _bytes(c.prob.circuit_get()) == _bytes(s)


# ---- 2: the advance ---------------------------------------------------------------------------------------------------------
def _restate_advance(state_before, cap, dt, dt_old, V, R, Cp):
    """the restatement's advance from what the device held before the call"""
    return circ.advance(state_before.raw["conduction"], state_before.raw["conductance"], cap, state_before.U_old,
                        state_before.U_old1, dt, dt_old, V, R, Cp)


def _check_advance(what, got, want, before, cap, dt, dt_old, V, R, Cp):
    from fedm_amd.physical_constants import elementary_charge as e, epsilon_0 as eps0
    R, Cp, V = (np.asarray(a, dtype=np.float64) for a in (R, Cp, V))
    scale = tc.voltage_scale(V, before.U_old, before.U_old1)
    a, b, c_ = circ.bdf2(dt, dt_old)
    drv = R > 0.0
    cond_A = 1.0
    if drv.any():
        M = a * eps0 * np.asarray(cap) + e * before.raw["conductance"]
        cond_A = float(np.linalg.cond(M[np.ix_(drv, drv)] + np.diag(1.0 / R[drv] + a * Cp[drv])))
    dU = float(np.abs(got.U - want["U"]).max()) / scale
    rate_scale = a * np.abs(want["U"]) + np.abs(b * before.U_old) + np.abs(c_ * before.U_old1)
    dR = float((np.abs(got.dUdt - want["dUdt"]) / rate_scale).max())
    lead_scale = np.where(drv, (np.abs(V) + np.abs(want["U"])) / np.where(drv, R, 1.0),
                          e * np.abs(before.raw["conduction"]) + e * np.abs(before.raw["conductance"]) @ (np.abs(want["U"]) + np.abs(before.U_old))
                          + eps0 * np.abs(cap) @ rate_scale + Cp * rate_scale)
    dL = float((np.abs(got.lead_current - want["lead"]) / lead_scale).max())
    print(f"[circuit] advance {what}: condition {cond_A:.1f}, |U - restated| / max voltage {dU:.2e}, dU/dt {dR:.2e}, "
          f"lead current {dL:.2e} of their sums of |terms|", flush=True)
    assert got.flag == 0
    assert dU <= ADVANCE_BOUND and dR <= ADVANCE_BOUND and dL <= ADVANCE_BOUND, (what, dU, dR, dL)


def _two_steps(c, k):
    """set-up, measure, the first step (FIRST_STEP), measure: the device with a history; returns the capacitance"""
    n = len(k["R"])
    c.reset()
    c.prob.currents_setup(potentials=c.potentials(n))
    cap = c.prob.currents().raw["capacitance"]
    c.prob.circuit_setup(k["R"], k["Cp"], k["U0"], electrode_of_entry=_no_entries(c.prob))
    c.prob.circuit_measure()
    before = c.prob.circuit_get()
    c.prob.set_step(*tc.FIRST_STEP)
    got = c.prob.circuit_advance(k["V_first"], read=True)
    return cap, before, got


@pytest.mark.parametrize("name", list(tc.ADVANCE_CASES))
def test_the_advance_against_the_restatement(cases, name):
    c = cases("a", "closed")
    k = tc.ADVANCE_CASES[name]
    try:
        cap, before, got = _two_steps(c, k)
        assert np.array_equal(before.U, k["U0"]) and np.array_equal(before.U_old1, k["U0"])
        want = _restate_advance(before, cap, *tc.FIRST_STEP, k["V_first"], k["R"], k["Cp"])
        _check_advance(f"{name!r}, the first step (dt_old = 1e30)", got, want, before, cap, *tc.FIRST_STEP, k["V_first"], k["R"], k["Cp"])
        for g, r in enumerate(k["R"]):
            if r == 0.0:
                assert got.U[g] == k["V_first"][g]                 # an ideal source: bitwise
        c.prob.circuit_measure()
        before = c.prob.circuit_get()
        assert np.array_equal(before.U_old, got.U) and np.array_equal(before.U_old1, k["U0"])
        c.prob.set_step(c.c.dt, c.c.dt_old)
        second = c.prob.circuit_advance(k["V"], read=True)
        want = _restate_advance(before, cap, c.c.dt, c.c.dt_old, k["V"], k["R"], k["Cp"])
        _check_advance(f"{name!r}, the second step", second, want, before, cap, c.c.dt, c.c.dt_old, k["V"], k["R"], k["Cp"])
        # a retried step: another dt from the same measure, then the first dt again and a fresh run of the same calls
        c.prob.set_step(0.4 * c.c.dt, c.c.dt_old)
        retried = c.prob.circuit_advance(k["V"], read=True)
        want = _restate_advance(before, cap, 0.4 * c.c.dt, c.c.dt_old, k["V"], k["R"], k["Cp"])
        _check_advance(f"{name!r}, retried with 0.4 dt", retried, want, before, cap, 0.4 * c.c.dt, c.c.dt_old, k["V"], k["R"], k["Cp"])
        assert np.array_equal(retried.U_old, before.U_old) and np.array_equal(retried.U_old1, before.U_old1)
        assert not np.array_equal(retried.U, second.U)
        c.prob.set_step(c.c.dt, c.c.dt_old)
        assert _bytes(c.prob.circuit_advance(k["V"], read=True)) == _bytes(second)
        _two_steps(c, k)
        c.prob.circuit_measure()
        c.prob.set_step(0.4 * c.c.dt, c.c.dt_old)
        assert _bytes(c.prob.circuit_advance(k["V"], read=True)) == _bytes(retried)
        assert c.prob.circuit_advance(k["V"]) is None and _bytes(c.prob.circuit_get()) == _bytes(retried)
    finally:
        c.reset()


def _crossed(kind):
    c = tc.crossed_case(kind)
    prob = tr.device_streamer_problem(c.mesh.coords, c.mesh.cells, c.dm)
    prob.set_state(c.U, c.U, c.U)
    return c, prob


def test_the_solve_takes_the_electrodes_potential_bitwise():
    c, prob = _crossed("plasma")
    try:
        from fedm_amd.device import boundary_vertex_groups
        group = boundary_vertex_groups(prob.cells, prob.facet_tags(), prob.nv, prob.dirichlet_vertices(), (1, 2))
        dd = prob._ddofs.astype(np.int64)
        vertex = prob._order[dd // 3]
        entry = np.where(group[vertex] == 2, 1, -1).astype(np.int8)         # the anode's entries alone
        assert (entry == 1).sum() == 11 and (entry == -1).sum() == 11
        uploaded = np.where(group[vertex] == 1, 3.25, 7.0)
        prob.set_dirichlet_values(uploaded)
        prob.currents_setup(boundary_tags=(1, 2), rtol=tgc.RTOL)
        prob.circuit_setup([0.0, tc.STABILITY["R"]], [0.0, 1e-13], [3.25, tc.STABILITY["U_anode"]], electrode_of_entry=entry)
        prob.circuit_measure()
        prob.shift_state()
        prob.set_step(1e-11, 1e30)
        s = prob.circuit_advance([3.25, 18000.0], read=True)
        assert s.flag == 0 and s.U[0] == 3.25 and s.U[1] not in (7.0, 18000.0, tc.STABILITY["U_anode"])
        prob.newton_solve(rtol=1e-6, max_it=20)
        Phi = prob.get_state()[:, 2]
        assert np.array_equal(Phi[group == 2], np.full(11, s.U[1]))
        assert np.array_equal(Phi[group == 1], np.full(11, 3.25))
    finally:
        prob.close()


# ---- 3: a vacuum gap charges as a capacitor; the signs --------------------------------------------------------------------------
def test_vacuum_gap_charges_through_the_resistor():
    """MEASURED on the MI355X: worst |U - restated| / V 1.02e-15 over the 20 steps; worst Kirchhoff mismatch against the
    displacement form of fedm_currents 3.57e-13 of the sum of the magnitudes (bound 1e-8), at the anode and, with the other
    sign, at the ideal cathode; U(2 RC) 878.0895 V against the exact 878.1982 V."""
    from fedm_amd.physical_constants import epsilon_0
    c, prob = _crossed("vacuum")
    try:
        prob.currents_setup(boundary_tags=(1, 2), rtol=1e-12)
        cap = prob.currents().raw["capacitance"]
        Cp, V = 2.0e-13, 1000.0
        Ctot = epsilon_0 * cap[1, 1] + Cp
        R = 1.0e-9 / Ctot                                   # RC = 1 ns
        dt = R * Ctot / 10.0
        U0 = tc.VACUUM_U0
        prob.circuit_setup([0.0, R], [0.0, Cp], [0.0, U0], boundary_tags=(1, 2))
        prob.circuit_measure()
        U_ref, dt_old, worst_u, worst_k = [U0, U0], 1e30, 0.0, 0.0
        zeros = np.zeros((2, 2))
        for step in range(20):
            prob.shift_state()
            prob.set_step(dt, dt_old)
            s = prob.circuit_advance([0.0, V], read=True)
            want = circ.advance([0.0, 0.0], zeros, cap, [0.0, U_ref[0]], [0.0, U_ref[1]], dt, dt_old, [0.0, V], [0.0, R], [0.0, Cp])
            U_ref = [float(want["U"][1]), U_ref[0]]
            worst_u = max(worst_u, abs(s.U[1] - U_ref[0]) / V)
            assert s.flag == 0 and s.U[0] == 0.0
            prob.newton_solve(rtol=NEWTON_RTOL, atol=0.0, max_it=50, ksp_rtol=1e-8)
            cur = prob.currents()
            kirchhoff = (V - s.U[1]) / R - Cp * s.dUdt[1]
            scale = abs(V - s.U[1]) / R + Cp * abs(s.dUdt[1])
            miss = [abs(kirchhoff - cur.total[1]) / scale, abs(s.lead_current[0] - cur.total[0]) / scale]
            worst_k = max(worst_k, *miss)
            if step in (0, 1, 19):
                print(f"[circuit] vacuum step {step + 1}: U {s.U[1]:.9f} V (restated {U_ref[0]:.9f}), (V - U)/R - Cp D_tU "
                      f"{kirchhoff:.9e} A, fedm_currents total {cur.total[1]:.9e} A, at the cathode {cur.total[0]:.9e} A",
                      flush=True)
            assert cur.finite and abs(cur.conduction[1]) <= 1e-30 * scale
            prob.circuit_measure()
            dt_old = dt
        exact = V - (V - U0) * math.exp(-2.0)
        print(f"[circuit] vacuum RC, 20 steps of RC/10: worst |U - restated| / V {worst_u:.2e}, worst Kirchhoff mismatch "
              f"{worst_k:.2e} (bound {CLOSURE_BOUND:.0e}); U(2 RC) {s.U[1]:.6f} V, V - (V - U0) exp(-2) {exact:.6f} V", flush=True)
        assert worst_u <= 1e-12
        assert worst_k <= CLOSURE_BOUND
        assert abs(s.U[1] - exact) <= 1e-3 * V and s.U[1] > 0.8 * V > U0           # the capacitor charges: the signs
    finally:
        prob.close()


# ---- 4: with a plasma, against a host run of the same algorithm --------------------------------------------------------------
def _kirchhoff_mismatch(prob, s, V, R, Cp):
    cur = prob.currents()
    lhs = (V - s.U[1]) / R - Cp * s.dUdt[1]
    return abs(lhs - cur.total[1]) / (abs(lhs) + abs(cur.total[1]))


def test_five_steps_with_a_plasma_against_the_host():
    """MEASURED on the MI355X: states within 5.5e-14 of each component's largest value, U within 5.6e-15 (bound 1e-9); the
    lagged Kirchhoff mismatch of the first step 1.512e-2 at dt and 7.561e-3 at dt / 2 (printed, not asserted)."""
    from oracle.newton import newton_solve
    from fedm_amd.physical_constants import elementary_charge as e
    k = tc.STABILITY
    c, prob = _crossed("plasma")
    try:
        om, R, Cp, dt = c.om, k["R"], 1.0e-13, k["dt"]
        psis = tc.electrode_potentials(c)
        prob.currents_setup(boundary_tags=(1, 2), rtol=1e-12)
        cap = prob.currents().raw["capacitance"]
        assert np.abs(prob.currents_psi() - psis).max() <= 1e-9
        ref0 = cref.lfa_reference(om, c.U, c.U, c.U, dt, 1e30, psis)
        Vs = k["U_anode"] + R * e * ref0["conduction"][1].value          # the source that holds the gap where it starts
        prob.circuit_setup([0.0, R], [0.0, Cp], [0.0, k["U_anode"]], boundary_tags=(1, 2))
        prob.circuit_measure()
        # the host: the oracle's Newton step with the Dirichlet values of the restated advance
        Uh, Uh_old, Uh_old1 = c.U.copy(), c.U.copy(), c.U.copy()
        hist = [np.array([0.0, k["U_anode"]])] * 2
        anode = om.dirichlet_vals != 0.0
        dt_old, lag = 1e30, []
        for step in range(k["steps"]):
            refm = cref.lfa_reference(om, Uh, Uh_old, Uh_old1, dt, dt_old, psis)
            cond = np.array([x.value for x in refm["conduction"]])
            G = circ.values(circ.lfa_conductance(om, Uh, psis))
            want = circ.advance(cond, G, cap, hist[0], hist[1], dt, dt_old, [0.0, Vs], [0.0, R], [0.0, Cp])
            hist = [want["U"], hist[0]]
            Uh_old1, Uh_old = Uh_old, Uh.copy()
            om.dirichlet_vals = np.where(anode, want["U"][1], 0.0)
            newton_solve(om, Uh, Uh_old, Uh_old1, dt, dt_old, 1e-8, 25)
            prob.shift_state()
            prob.set_step(dt, dt_old)
            s = prob.circuit_advance([0.0, Vs], read=True)
            prob.newton_solve(rtol=1e-8, max_it=25, ksp_rtol=1e-10)
            Ud = prob.get_state()
            d = np.abs(Ud - Uh).max(axis=0) / np.abs(Uh).max(axis=0)
            dU = abs(s.U[1] - want["U"][1]) / abs(want["U"][1])
            lag.append(_kirchhoff_mismatch(prob, s, Vs, R, Cp))
            print(f"[circuit] plasma step {step + 1}: U {s.U[1]:.6f} V (host {want['U'][1]:.6f}), |U - host| / U {dU:.2e}, "
                  f"states {d.max():.2e}, lagged Kirchhoff mismatch {lag[-1]:.2e}", flush=True)
            assert s.flag == 0 and d.max() <= PARITY_BOUND and dU <= PARITY_BOUND, (step, d, dU)
            prob.circuit_measure()
            dt_old = dt
        # (printed, not asserted) the first-order lag: the same start with half the step
        prob.set_state(c.U, c.U, c.U)
        prob.circuit_setup([0.0, R], [0.0, Cp], [0.0, k["U_anode"]], boundary_tags=(1, 2))
        prob.circuit_measure()
        prob.shift_state()
        prob.set_step(0.5 * dt, 1e30)
        s = prob.circuit_advance([0.0, Vs], read=True)
        prob.newton_solve(rtol=1e-8, max_it=25, ksp_rtol=1e-10)
        print(f"[circuit] lagged Kirchhoff mismatch of the first step at dt {lag[0]:.3e}, at dt / 2 "
              f"{_kirchhoff_mismatch(prob, s, Vs, R, Cp):.3e}", flush=True)
    finally:
        prob.close()


# ---- 5: without a circuit nothing has changed ---------------------------------------------------------------------------------
def test_the_glow_case_without_a_circuit_gives_the_parents_bytes():
    """tests/golden/circuit_glow_none_state.npy: the state after three steps of Case(nx=8, ny=8) as the parent commit's
    tree left it on an MI355X (recorded beside two runs of this tree, which gave the same bytes)."""
    from fedm_amd.cases import glow_discharge as gdc
    want = np.load(ROOT / "tests" / "golden" / "circuit_glow_none_state.npy")
    case = gdc.Case(nx=8, ny=8, T_final=1.0, circuit=None)
    try:
        assert case.circuit is None
        for _ in range(3):
            case.step()
        got = case.prob.get_state()
        print(f"[circuit] Case(circuit=None), three steps: max |state - parent's| {np.abs(got - want).max():.3e}", flush=True)
        assert got.tobytes() == want.tobytes()
        # ... and with one the powered electrode lags the source
        ballasted = gdc.Case(nx=8, ny=8, T_final=1.0, circuit=dict(resistance=1.0e5, capacitance=1.0e-12))
        try:
            for _ in range(3):
                ballasted.step()
            s = ballasted.circuit.state()
            Vs = ballasted.circuit.voltages(ballasted.t)[0]
            Phi = ballasted.prob.get_state()[ballasted.powered, -1]
            print(f"[circuit] Case(circuit=1e5 ohm, 1 pF), three steps: V_s {Vs:.6e} V, U {s.U_old[0]:.6e} V", flush=True)
            assert s.flag == 0 and 0.0 < abs(s.U_old[0]) < abs(Vs)
            # (the LMEA family's constrained rows take their value through the Newton update: to the case's Newton
            # tolerance, 1e-4, not bitwise)
            assert np.abs(Phi - s.U_old[0]).max() <= 1e-4 * abs(s.U_old[0])
        finally:
            ballasted.prob.close()
    finally:
        case.prob.close()


# ---- 6: the example's log ---------------------------------------------------------------------------------------------------
def _example(name):
    spec = importlib.util.spec_from_file_location(f"{name}_example_circuit", ROOT / "examples" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_glow_example_writes_the_circuit_log(tmp_path):
    mod = _example("glow_discharge")
    out = tmp_path / "circuit.txt"
    res = mod.main(nx=8, ny=8, T_final=2e-11, output_dir=tmp_path / "run", ballast=1.0e5, stray_capacitance=1.0e-12,
                   circuit_log=out)
    assert out.read_text().splitlines()[0].split() == ["#", *mod.CIRCUIT_COLUMNS]
    assert mod.CIRCUIT_COLUMNS == ("t", "V_s", "U", "lead_current", "conduction", "conductance")
    rows = np.atleast_2d(np.loadtxt(out))
    print(f"[circuit] glow example, ballast 1e5 ohm: rows\n{rows}", flush=True)
    assert rows.shape == (res["steps"], len(mod.CIRCUIT_COLUMNS)) and rows.shape[0] >= 3
    assert np.isfinite(rows).all() and np.all(np.diff(rows[:, 0]) > 0.0)
    assert np.all(rows[:, 5] > 0.0) and np.all(np.abs(rows[:, 2]) <= np.abs(rows[:, 1]))      # G > 0; |U| lags |V_s|


def test_the_streamer_example_writes_the_circuit_log(tmp_path):
    mod = _example("streamer_discharge")
    out = tmp_path / "circuit.txt"
    mod.main(cells=12, end_time=1.5e-11, output_dir=tmp_path / "run", quiet=True, ballast=1.0e3, circuit_log=out)
    assert out.read_text().splitlines()[0].split() == ["#", *mod.CIRCUIT_COLUMNS]
    rows = np.atleast_2d(np.loadtxt(out))
    print(f"[circuit] streamer example, ballast 1e3 ohm: rows\n{rows}", flush=True)
    assert rows.shape == (3, len(mod.CIRCUIT_COLUMNS)) and np.isfinite(rows).all()
    assert np.all(rows[:, 5] > 0.0) and np.all(rows[:, 1] == 18750.0)


# ---- 7: refusals and the flag -----------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(cases):
    from fedm_amd import _lib
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))          # noqa: E731
    V = np.zeros(8)
    for key in (("a", "closed"), ("ion-e", "3x3", False)):
        c = cases(*key)
        c.reset()
        lib, h = c.prob.lib, c.prob._h
        c.prob.currents_setup(potentials=c.potentials(2))
        entry = _no_entries(c.prob)

        def desc(n=2, R=(1.0, 0.0), Cp=(0.0, 0.0), U0=(0.0, 0.0), e=entry):
            d = _lib.CircuitDesc()
            d.n = n
            for g in range(2):
                d.R[g], d.Cp[g], d.U0[g] = R[g], Cp[g], U0[g]
            d.electrode_of_entry = e.ctypes.data_as(C.POINTER(C.c_int8)) if e is not None else None
            return d
        assert lib.fedm_circuit_setup(h, None) == -2 and "null" in _lib.last_error()
        assert lib.fedm_circuit_setup(h, C.byref(desc(n=3))) == -2 and "3 electrodes" in _lib.last_error()
        for bad in (-1.0, np.nan, np.inf):
            assert lib.fedm_circuit_setup(h, C.byref(desc(R=(1.0, bad)))) == -2 and "R[1]" in _lib.last_error()
            assert lib.fedm_circuit_setup(h, C.byref(desc(Cp=(bad, 0.0)))) == -2 and "Cp[0]" in _lib.last_error()
        assert lib.fedm_circuit_setup(h, C.byref(desc(U0=(0.0, np.nan)))) == -2 and "U0[1]" in _lib.last_error()
        assert lib.fedm_circuit_setup(h, C.byref(desc(e=None))) == -2 and "null" in _lib.last_error()
        for bad in (2, -2):
            wrong = entry.copy()
            wrong[3] = bad
            assert lib.fedm_circuit_setup(h, C.byref(desc(e=wrong))) == -2 and "electrode_of_entry[3]" in _lib.last_error()
        assert lib.fedm_circuit_setup(h, C.byref(desc())) == 0
        out = _lib.CircuitState()
        assert lib.fedm_circuit_advance(h, dp(V), C.byref(out)) == -2 and "fedm_circuit_measure has not" in _lib.last_error()
        assert lib.fedm_circuit_get(h, None) == -2 and "null" in _lib.last_error()
        assert lib.fedm_circuit_measure(h) == 0
        assert lib.fedm_circuit_advance(h, None, C.byref(out)) == -2 and "null" in _lib.last_error()
        assert lib.fedm_circuit_advance(h, dp(V), C.byref(out)) == 0 and out.flag == 0 and out.n == 2
        # a refused set-up leaves the one in force; the currents set-up changing its count is seen
        assert lib.fedm_circuit_setup(h, C.byref(desc(n=3))) == -2
        assert lib.fedm_circuit_advance(h, dp(V), C.byref(out)) == 0
        c.prob.currents_setup(potentials=c.potentials(3))
        assert lib.fedm_circuit_measure(h) == -2 and "changed" in _lib.last_error()
        with pytest.raises(ValueError, match="either"):
            c.prob.circuit_setup(1.0)
        with pytest.raises(ValueError, match="3 electrodes"):
            c.prob.circuit_setup([1.0, 2.0], electrode_of_entry=entry)
    # before a set-up
    m = streamer.mesh(4)
    fresh = streamer.device_problem(m.coords, m.cells)
    try:
        out = _lib.CircuitState()
        d = _lib.CircuitDesc()
        d.n = 1
        assert fresh.lib.fedm_circuit_setup(fresh._h, C.byref(d)) == -2 and "fedm_currents_setup has not" in _lib.last_error()
        assert fresh.lib.fedm_circuit_measure(fresh._h) == -2 and "fedm_circuit_setup has not" in _lib.last_error()
        assert fresh.lib.fedm_circuit_advance(fresh._h, dp(V), None) == -2 and "fedm_circuit_setup has not" in _lib.last_error()
        assert fresh.lib.fedm_circuit_get(fresh._h, C.byref(out)) == -2 and "fedm_circuit_setup has not" in _lib.last_error()
        with pytest.raises(RuntimeError, match="currents_setup has not"):
            fresh.circuit_setup(1.0, boundary_tags=(1, 2))
    finally:
        fresh.close()
    # no Poisson equation
    msh = Mesh(m.coords, m.cells)
    dm = Model(n_species=1, poisson=False, eq_type=["diffusion-reaction"], Z=[-1.0], D=[TermSum.const(0.1)],
               reactions=[Reaction(TermSum.const(1.0), power=[1], net=[1])], bc_kind=[["zero flux"]] * 4, quadrature_degree=2)
    plain = DeviceProblem(msh.coords, msh.cells, dm, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES))
    try:
        d = _lib.CircuitDesc()
        d.n = 1
        assert plain.lib.fedm_circuit_setup(plain._h, C.byref(d)) == -2 and "Poisson" in _lib.last_error()
    finally:
        plain.close()


def test_a_context_with_ghosts_is_refused(cases):
    from fedm_amd import _lib
    from fedm_amd.device import DeviceProblem
    c = cases("ion-e", "3x3", False)
    cc = c.c.c
    prob = DeviceProblem(c.c.mesh.coords, c.c.mesh.cells, c.c.model, facet_tags=c.c.mesh.tags, dirichlet_dofs=cc.dirichlet_dofs,
                         dirichlet_vals=cc.dirichlet_vals, n_owned=c.c.mesh.nv - 3)
    try:
        d = _lib.CircuitDesc()
        d.n = 1
        assert prob.lib.fedm_circuit_setup(prob._h, C.byref(d)) == -2 and "ghost" in _lib.last_error()
    finally:
        prob.close()


@pytest.mark.parametrize("key", [("a", "closed"), ("ion-e", "3x3", False)])
def test_a_state_that_is_not_finite_sets_the_flag_and_leaves_u(cases, key):
    c = cases(*key)
    c.reset()
    k = tc.ADVANCE_CASES["one ideal of two"]
    try:
        _two_steps(c, k)
        c.prob.circuit_measure()
        c.prob.set_step(c.c.dt, c.c.dt_old)
        good = c.prob.circuit_advance(k["V"], read=True)
        assert good.flag == 0
        bad = c.c.U.copy()
        bad[c.prob.nv // 2, c.prob.n_eq - 1] = np.nan
        c.prob.set_state(u_new=bad)
        c.prob.circuit_measure()
        flagged = c.prob.circuit_advance([5.0, 6.0], read=True)
        # (FEDM_CIRCUIT_NOT_FINITE; a NaN conductance makes the pivot not finite as well)
        assert flagged.flag & 1 and np.array_equal(flagged.U, good.U) and np.array_equal(flagged.U_old, good.U)
        c.reset()
        c.prob.circuit_measure()
        clean = c.prob.circuit_advance(k["V"], read=True)
        assert clean.flag == 0 and np.isfinite(clean.U).all() and np.array_equal(clean.U_old, good.U)
        assert np.array_equal(clean.raw["conductance"], good.raw["conductance"])
    finally:
        c.reset()
