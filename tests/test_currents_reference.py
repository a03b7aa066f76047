"""tests/currents_reference.py, the numpy restatement of the electrode currents, pinned on closed forms, on the two older
restatements' induced current, and shown to see deliberate faults at the bound the device is held to (no GPU).

The cases of tests/test_gpu_currents.py are made here (``lfa_case``, ``lmea_case``): meshes and models of
tests/test_gpu_diagnostics.py and tests/lmea_models.py, three different states -- the densities perturbed as those tests
perturb them, the potential of the two older states 0.8 and 0.55 of the new one plus noise, a rising voltage, so that
D_t Phi is no cancellation of noise -- and dt != dt_old.
"""
import dataclasses
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import balance_reference as bref  # noqa: E402
import currents_reference as cref  # noqa: E402
import diagnostics_reference as dref  # noqa: E402

DEVICE_BOUND = 1e-12          # tests/test_gpu_currents.py: |device - fsum| <= 1e-12 sum |terms|
LFA_DT, LFA_DT_OLD = 3e-12, 5e-12


def _older(U, seed, iphi):
    """The two older states of U: everything perturbed a little, the potential 0.8 and 0.55 of the new one plus noise."""
    rng = np.random.default_rng(seed)
    scale = np.abs(U[:, iphi]).max()
    out = []
    for f in (0.8, 0.55):
        V = U.copy()
        noise = rng.normal(0, 0.02, (U.shape[0], iphi))
        densities = np.abs(U[:, :iphi]).max(axis=0) > 100.0        # a linear representation: 2 % of the value
        V[:, :iphi] += np.where(densities, noise * U[:, :iphi], noise)
        V[:, iphi] = f * U[:, iphi] + rng.normal(0, 1e-3 * scale, U.shape[0])
        out.append(V)
    return out


_LFA = {}


def lfa_case(mesh_name, kind):
    """namespace(om, dm, mesh, U, Uo, Uo1, dt, dt_old, box) of an LFA model on a mesh of tests/test_gpu_diagnostics.py.
    kind: "closed", "planar", "tabulated" (its ``_models``), "linear" (tests/test_oracle_linear.py's model), "reaction"
    (the streamer with an ion of the 'reaction' type that has a mobility and a diffusion coefficient all the same: its
    flux is 0 by its type alone).  Made once, read-only."""
    import test_gpu_diagnostics as tgd
    from oracle import streamer as ost
    if (mesh_name, kind) in _LFA:
        return _LFA[mesh_name, kind]
    mesh = tgd._mesh(mesh_name)
    if kind == "linear":
        from test_oracle_linear import _model, _state
        from fedm_amd.cases import streamer
        om = _model(mesh, log=False)
        lnn, phi = _state(mesh, seed=9)
        U = np.column_stack([np.exp(lnn), phi])
        dm = dataclasses.replace(streamer.model(), log_representation=False)
    elif kind == "reaction":
        from oracle.forms import LFAModel
        from oracle.mesh import mark_boundaries
        from fedm_amd.cases import streamer
        from fedm_amd.termsum import TermSum
        om = LFAModel(mesh, n_species=2, poisson=True, eq_type=["reaction", "drift-diffusion-reaction"], Z=[1.0, -1.0],
                      mu=[2e-2, ost.MU_E], D=[3e-2, ost.D_E], reactions=[(ost.K_ION, [0, 1], [1, 1])],
                      facet_tags=mark_boundaries(mesh, ost.BOUNDARIES), bc_type=ost.BC_TYPE, qdeg=2)
        base = streamer.model()
        dm = dataclasses.replace(base, mu=[TermSum.const(2e-2), base.mu[1]], D=[TermSum.const(3e-2), base.D[1]])
        U = tgd._models(mesh, "closed")[2]
    else:
        om, dm, U, _ = tgd._models(mesh, kind)
    Uo, Uo1 = _older(U, 41, om.ns)
    c = types.SimpleNamespace(om=om, dm=dm, mesh=mesh, U=U, Uo=Uo, Uo1=Uo1, dt=LFA_DT, dt_old=LFA_DT_OLD, box=ost.BOX,
                              kind=kind, r0=0.0)
    for a in (U, Uo, Uo1):
        a.setflags(write=False)
    _LFA[mesh_name, kind] = c
    return c


def lfa_restate(c, psis, faults=(), states=None):
    U, Uo, Uo1 = states or (c.U, c.Uo, c.Uo1)
    return cref.lfa_reference(c.om, U, Uo, Uo1, c.dt, c.dt_old, psis, faults)


_LMEA = {}


def lmea_case(name, mesh_name="10x10", planar=False):
    """tests/lmea_models.case with the older states' potentials replaced (``_older``): namespace(c, U, Uo, Uo1, ...)."""
    import lmea_models as lm
    if (name, mesh_name, planar) in _LMEA:
        return _LMEA[name, mesh_name, planar]
    c = lm.case(name, mesh_name, planar)
    ns = c.model.n_species
    Uo, Uo1 = _older(c.U, 43, ns)
    out = types.SimpleNamespace(c=c, md=c.md, model=c.model, mesh=c.mesh, fields=c.fields, U=c.U, Uo=Uo, Uo1=Uo1, dt=c.dt,
                                dt_old=c.dt_old, box=c.mesh.L, r0=lm.R0, planar=planar, name=name)
    for a in (Uo, Uo1):
        a.setflags(write=False)
    _LMEA[name, mesh_name, planar] = out
    return out


def lmea_restate(c, psis, faults=(), states=None):
    U, Uo, Uo1 = states or (c.U, c.Uo, c.Uo1)
    return cref.lmea_reference(c.md, c.mesh.coords, c.mesh.cells, c.fields, U, Uo, Uo1, c.dt, c.dt_old, c.c.rules[0], psis,
                               faults=faults)


# ---- closed forms ----------------------------------------------------------------------------------------------------------
def _volume(c, lmea, planar):
    """(capacitance of psi = z / d, volume) of the rectangle: pi R^2 / d and width / d."""
    d = c.box
    if planar:
        return d / d, d * d
    r0, r1 = c.r0, c.r0 + d
    return np.pi * (r1 * r1 - r0 * r0) / d, np.pi * (r1 * r1 - r0 * r0) * d


@pytest.mark.parametrize("family,planar", [("lfa", False), ("lfa", True), ("lmea", False), ("lmea", True)])
def test_closed_forms(family, planar):
    lmea = family == "lmea"
    c = lmea_case("e-only", "10x10", planar) if lmea else lfa_case("b", "planar" if planar else "closed")
    restate = lmea_restate if lmea else lfa_restate
    z = c.mesh.coords[:, 1]
    psi = z / c.box
    iphi = c.U.shape[1] - 1
    cap, vol = _volume(c, lmea, planar)
    # Phi = V(t_k) z / d at three unequal times, uniform densities
    V = (-250.0, -180.0, -75.0)
    n = [3.0e14, 2.0e14]
    states = []
    for Vk in V:
        S = c.U.copy()
        S[:, iphi] = Vk * psi
        if lmea:
            S[:, 1] = np.log(n[1])
        else:
            S[:, 0], S[:, 1] = np.log(n[0]), np.log(n[1])
        states.append(S)
    ref = restate(c, psi[None, :], states=tuple(states))
    got = ref["capacitance"][0][0]
    print(f"[currents reference] {family} planar={planar}: capacitance {got.value!r} closed form {cap!r}")
    assert abs(got.value - cap) <= 1e-13 * cap
    w = c.dt / c.dt_old
    DtV = ((1 + 2 * w) * V[0] - (1 + w) ** 2 * V[1] + w * w * V[2]) / ((1 + w) * c.dt)
    assert abs(ref["displacement"][0].value - cap * DtV) <= 1e-12 * ref["displacement"][0].abs
    assert abs(ref["coupling"][0].value - cap * V[0]) <= 1e-12 * ref["coupling"][0].abs
    charge = (-n[1] if lmea else n[0] - n[1]) * vol / 2.0
    assert abs(ref["induced_charge"][0].value - charge) <= 1e-12 * ref["induced_charge"][0].abs
    # the variable-step weights sum to 0 and reproduce a linear ramp's slope
    cw = cref.bdf2_weights(c.dt, c.dt_old)
    assert abs(cw.sum()) <= 4e-16 * np.abs(cw).sum()
    assert abs(cw[1] * (-c.dt) + cw[2] * (-c.dt - c.dt_old) - 1.0) <= 1e-15


@pytest.mark.parametrize("kind", ["closed", "planar", "linear", "reaction"])
def test_conduction_is_the_diagnostics_induced_current(kind):
    c = lfa_case("b", kind)
    psi = cref.test_potentials(c.mesh.coords, c.box, 1)
    ref = lfa_restate(c, psi)
    old = dref.reference(c.om, c.U, psi=psi[0])["current"]
    print(f"[currents reference] LFA {kind}: conduction {ref['conduction'][0].value!r} induced_current {old.value!r}")
    assert old.value != 0.0
    assert abs(ref["conduction"][0].value - old.value) <= 1e-14 * old.abs


@pytest.mark.parametrize("name,planar", [("e-only", True), ("ion-e", False), ("deck-shape-permuted", False),
                                         ("two-ions-small", True), ("two-ions-full", False)])
def test_conduction_is_the_balance_induced_current(name, planar):
    c = lmea_case(name, "10x10", planar)
    psi = cref.test_potentials(c.mesh.coords, c.box, 1, c.r0)
    ref = lmea_restate(c, psi)
    cc = c.c
    old = bref.reference(c.md, c.mesh.coords, c.mesh.cells, c.mesh.tags, c.fields, c.U, c.Uo, c.Uo1, c.dt, c.dt_old,
                         cc.rules[0], cc.rules[1], psi=psi[0])["induced_current"]
    assert old.value != 0.0
    assert abs(ref["conduction"][0].value - old.value) <= 1e-14 * old.abs


# ---- the bound sees deliberate faults, and no output is a sum of zeros ----------------------------------------------------
FAULT_CASES = [("equal-step BDF2 weights", "lfa", "closed", "displacement"),
               ("equal-step BDF2 weights", "lmea", "two-ions-small", "displacement"),
               ("u_old1 taken for u_old", "lfa", "closed", "displacement"),
               ("u_old1 taken for u_old", "lmea", "two-ions-small", "displacement"),
               ("+grad psi", "lfa", "closed", "conduction"),
               ("+grad psi", "lmea", "two-ions-small", "conduction"),
               ("a reaction species' flux kept", "lfa", "reaction", "conduction"),
               ("sign_s left out", "lmea", "two-ions-small", "conduction"),
               ("sign_s left out", "lmea", "two-ions-small", "induced_charge"),
               ("planar weight taken as 1", "lfa", "planar", "capacitance"),
               ("planar weight taken as 1", "lmea", "two-ions-small", "conduction")]


def _fault_case(family, which):
    if family == "lfa":
        c = lfa_case("b", which)
        return c, lfa_restate, cref.test_potentials(c.mesh.coords, c.box, 3)
    c = lmea_case(which, "10x10", True)
    return c, lmea_restate, cref.test_potentials(c.mesh.coords, c.box, 3, c.r0)


@pytest.mark.parametrize("fault,family,which,output", FAULT_CASES)
def test_each_fault_misses_the_device_bound_by_a_factor_of_100(fault, family, which, output):
    assert fault in cref.FAULTS
    c, restate, psis = _fault_case(family, which)
    good, bad = restate(c, psis), restate(c, psis, faults=(fault,))
    pairs = ([(good[output][g][h], bad[output][g][h]) for g in range(3) for h in range(3)] if output == "capacitance"
             else list(zip(good[output], bad[output])))
    for g, (a, b) in enumerate(pairs):
        miss = abs(b.value - a.value) / (DEVICE_BOUND * a.abs)
        print(f"[currents reference] {fault!r} on {family} {which}: {output}[{g}] misses the bound {miss:.3g} times")
        assert miss >= 100.0, (fault, output, g, miss)


def test_the_six_faults_are_all_shown():
    assert {f for f, *_ in FAULT_CASES} == set(cref.FAULTS) and len(cref.FAULTS) >= 6


@pytest.mark.parametrize("family,which", [("lfa", "closed"), ("lfa", "planar"), ("lfa", "reaction"), ("lmea", "two-ions-small")])
def test_no_output_is_a_sum_of_zeros(family, which):
    c, restate, psis = _fault_case(family, which)
    ref = restate(c, psis)
    sums = [(f"{k}[{g}]", s) for k in cref.OUTPUTS for g, s in enumerate(ref[k])]
    sums += [(f"capacitance[{g}][{h}]", ref["capacitance"][g][h]) for g in range(3) for h in range(3)]
    for name, s in sums:
        print(f"[currents reference] {family} {which}: {name} |sum| / sum|terms| {abs(s.value) / s.abs:.3g}")
    for name, s in sums:
        assert abs(s.value) >= 1e-3 * s.abs, (name, s)
    cap = np.array([[ref["capacitance"][g][h].value for h in range(3)] for g in range(3)])
    assert np.array_equal(cap, cap.T) and np.linalg.matrix_rank(cap) == 3      # no two potentials are proportional


# ---- the bindings ----------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_bound_under_abi_10():
    import ctypes as C
    from fedm_amd import _lib
    for name in ("fedm_currents_setup", "fedm_currents_solve", "fedm_currents_get_psi", "fedm_currents"):
        assert name in _lib.exported_symbols()
    assert C.sizeof(_lib.CurrentsOut) == 8 * (4 * 8 + 64) + 8 and _lib.CURRENTS_MAX == 8
    header = (Path(__file__).resolve().parent.parent / "include" / "fedm_hip.h").read_text()
    assert "#define FEDM_ABI_VERSION 10" in header and "#define FEDM_CURRENTS_MAX 8" in header
    import fedm_amd.functions as ff
    assert callable(ff.Electrode_currents)


def test_electrode_currents_refuses_what_it_cannot_do():
    import fedm_amd.functions as ff
    dev = types.SimpleNamespace(model=types.SimpleNamespace(poisson=False))
    with pytest.raises(ValueError, match="Poisson"):
        ff.Electrode_currents(dev, boundary_tags=(1, 2))
    dev.model.poisson = True
    with pytest.raises(ValueError, match="either"):
        ff.Electrode_currents(dev)
    with pytest.raises(ValueError, match="either"):
        ff.Electrode_currents(dev, boundary_tags=(1,), weighting_potentials=np.zeros((1, 4)))
