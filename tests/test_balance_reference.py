"""tests/balance_reference.py pinned on the oracle's element residual and on closed forms (CPU), and the host-side checks
of the LMEA balance.

The identity: the P1 basis sums to 1 and its gradient to 0, and species and energy rows carry no Dirichlet condition, so
``element_residual(...).sum(axis=(0, 1))[c]`` -- the sum over all vertices of row c of the oracle's residual, which is
pinned on the reference's glow-discharge goldens -- equals ``rate_of_change[c] - source[c] + sum_t wall[t][c]`` of the
restatement, held here to ``1e-12 * sum |terms|`` of that row.  (The residual's flux terms ``W Gamma . grad phi_a`` cancel
over a = 0..2 to rounding only; they are 1e-4 .. 1e-5 of the BDF2 addends in ``sum |terms|``.)
"""
import math
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import balance_reference as bref  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
DECK = ROOT / "decks" / "glow_discharge" / "file_input" / "4_particles"
SENTINEL_LOSSES = [11.55, 7.77e77, -11.55, 4.21, -7.34, 0.0, 9.99e99]


def oracle_model(o, axisymmetric=True, degree=4):
    """The device model of fedm_amd.cases.glow_discharge.Case, from the oracle's deck (no device is touched)."""
    from fedm_amd.device import GdModel
    d = o.deck
    return GdModel(n_species=4, N0=o.N0, eq_type=["reaction", "diffusion-reaction", "drift-diffusion-reaction",
                                                 "drift-diffusion-reaction"],
                   grad_diffusion=[False, False, False, True], is_ion=[False, False, True, False], sign=list(d.sign),
                   vth=[0.0, o.vth_heavy[1], o.vth_heavy[2], 0.0], electron_mass=d.M[3], power=d.power.tolist(),
                   net=d.net.tolist(), energy_loss=list(d.energy_loss), energy_Ei=d.energy_Ei,
                   mean_energy_form="unknown_ratio", ref=[list(r) for r in o.ref], gamma=list(o.gamma),
                   we_secondary=o.we_met, quadrature_degree=degree, axisymmetric=axisymmetric)


def field_table(co, me_old, me, ue_old):
    """The nodal field table in the order of FEDM_GD_N_FIELDS from the oracle's coefficient dict."""
    nv = me_old.size
    zeros = np.zeros(nv)
    return np.stack(list(co["mu"]) + list(co["D"]) + [zeros] * 3 + [co["mu_e_diff"]] + [zeros] * 3 + [co["D_e_diff"]]
                    + list(co["k"]) + list(co["kd"]) + [me_old, me, ue_old])


def perturbed_case(losses="deck", degree=4):
    """The state and fields of tests/test_gpu_glow_discharge.py::_reference on the 10 x 10 crossed mesh."""
    from oracle import gd as ogd
    from oracle.quadrature import interval_rule, triangle_rule
    o = ogd.GlowDischarge(DECK, 10, 10)
    o.xq, o.wq = triangle_rule(degree)
    o.tq, o.wt = interval_rule(degree)
    if losses == "sentinels":
        o.deck.energy_loss, o.deck.energy_Ei = list(SENTINEL_LOSSES), 15.76
    nv = o.mesh.nv
    rng = np.random.default_rng(0)
    me_old = 3.0 + rng.normal(0, 0.3, nv)
    me = me_old + rng.normal(0, 0.05, nv)
    U = np.zeros((nv, 5))
    U[:, 0] = np.log(3.0) + np.log(1e12)
    U[:, 1:4] = np.log(1e12)
    U[:, 0] = np.log(me) + U[:, 3] + rng.normal(0, 0.05, nv)
    U[:, 1:4] += rng.normal(0, 0.2, (nv, 3))
    U[:, 4] = -100.0 * (1 - o.mesh.coords[:, 1] / 0.01) + rng.normal(0, 3.0, nv)
    Uo = U + rng.normal(0, 0.02, U.shape)
    Uo1 = U + rng.normal(0, 0.02, U.shape)
    co = o.coefficients(me_old, o.reduced_field(U[:, 4]))
    return types.SimpleNamespace(o=o, U=U, Uo=Uo, Uo1=Uo1, co=co, me_old=me_old, me=me, dt=1.1e-12, dt_old=0.7e-12,
                                 fields=field_table(co, me_old, me, Uo[:, 3]))


def restate(c, md, **kw):
    o = c.o
    return bref.reference(md, o.mesh.coords, o.mesh.cells, o.tags, c.fields, c.U, c.Uo, c.Uo1, c.dt, c.dt_old,
                          (o.xq, o.wq), (o.tq, o.wt), **kw)


@pytest.mark.parametrize("losses", ["deck", "sentinels"])
def test_the_imbalance_is_the_sum_of_the_oracles_residual_rows(losses):
    c = perturbed_case(losses)
    o = c.o
    assert o.mesh.nv == 221 and o.mesh.nc == 400
    md = oracle_model(o).to_c()
    ref = restate(c, md)
    cells = o.mesh.cells
    Re = o.element_residual(c.U[cells], c.Uo[cells], c.Uo1[cells], c.dt, c.dt_old, c.co, c.me_old, c.me, c.Uo[:, 3])
    rows = Re.sum(axis=(0, 1))
    for comp, imb in enumerate(bref.imbalance(ref)):
        ratio = abs(imb.value - rows[comp]) / imb.abs
        print(f"[balance] {losses} row {comp}: imbalance {imb.value:.6e} residual sum {rows[comp]:.6e} "
              f"|difference| / sum|terms| {ratio:.2e}")
        assert ratio <= 1e-12, (losses, comp, ratio)
        assert abs(imb.value) > 1e-6 * imb.abs        # the row's sum is no rounding residue: the check sees a wrong term
    if losses == "sentinels":
        assert ref["collision_loss"].value != restate(perturbed_case("deck"), oracle_model(perturbed_case("deck").o).to_c())[
            "collision_loss"].value


def _uniform_case(planar):
    from oracle import gd as ogd
    o = ogd.GlowDischarge(DECK, 10, 10)
    nv = o.mesh.nv
    n = [0.0, 2e12, 3e12, 5e12]
    z = o.mesh.coords[:, 1]
    U = np.zeros((nv, 5))
    U[:, 0] = math.log(3.0 * n[3])
    for i in (1, 2, 3):
        U[:, i] = math.log(n[i])
    U[:, 4] = -250.0 * (1.0 - z / o.gap)
    me = np.full(nv, 3.0)
    co = o.coefficients(me, o.reduced_field(U[:, 4]))
    c = types.SimpleNamespace(o=o, U=U, Uo=U.copy(), Uo1=U.copy(), co=co, me_old=me, me=me, dt=1e-12, dt_old=1e-12,
                              fields=field_table(co, me, me, U[:, 3]))
    return c, oracle_model(o, axisymmetric=not planar).to_c(), n


@pytest.mark.parametrize("planar", [False, True])
def test_closed_forms(planar):
    c, md, n = _uniform_case(planar)
    o = c.o
    ref = restate(c, md)
    volume = o.wall * o.gap if planar else math.pi * o.wall ** 2 * o.gap
    for i in (1, 2, 3):
        assert abs(ref["content"][i].value - n[i] * volume) <= 1e-12 * n[i] * volume
        assert abs(ref["content"][i].abs - n[i] * volume) <= 1e-12 * n[i] * volume      # every term is positive
    assert abs(ref["content"][0].value - 3.0 * n[3] * volume) <= 1e-12 * 3.0 * n[3] * volume
    # a linear potential: |grad Phi| = 250 V / gap in every cell
    assert abs(ref["field"].value - 250.0 / o.gap) <= 1e-12 * 250.0 / o.gap and 0 <= ref["field"].index < o.mesh.nc
    # u = u_old = u_old1: the BDF2 addends cancel to rounding, and are in sum |terms|
    for i in range(4):
        assert abs(ref["rate_of_change"][i].value) <= 1e-12 * ref["rate_of_change"][i].abs
    # tags 3 and 4 (axis, outer wall) reflect everything and emit nothing: exactly 0, and finite on the axis (r = 0)
    for t in (2, 3):
        for comp in range(4):
            assert ref["wall"][t][comp].value == 0.0 and ref["wall"][t][comp].plain == 0.0
    # the electrodes take particles; the gas (a 'reaction' species) has no wall term at all
    assert all(ref["wall"][t][0].abs > 0.0 and ref["wall"][t][2].value > 0.0 for t in (0, 1))
    # the switch overrides the model's flag
    other = restate(c, md, planar=not planar)
    assert abs(other["content"][1].value - n[1] * (math.pi * o.wall ** 2 * o.gap if planar else o.wall * o.gap)) \
        <= 1e-12 * other["content"][1].value
    # nodal maxima: uniform states tie, the lowest vertex is named
    assert ref["nodal"][3].value == c.U[0, 3] and ref["nodal"][3].index == 0 and not ref["nodal"][3].unique
    assert abs(ref["nodal"][4].value - math.log(3.0)) < 1e-14


# ---- host checks that need no GPU ---------------------------------------------------------------------------------------
def test_the_entry_points_are_bound_under_abi_10():
    import ctypes as C
    import re
    from fedm_amd import _lib
    assert _lib.ABI_VERSION == 10
    assert {"fedm_gd_balance_setup", "fedm_gd_balance"} <= set(_lib.exported_symbols())
    text = (ROOT / "include" / "fedm_hip.h").read_text()
    assert "#define FEDM_ABI_VERSION 10" in text
    body = re.search(r"struct fedm_gd_balance \{(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    consts = {"FEDM_GD_MAX_SPECIES": _lib.GD_MAX_SPECIES, "FEDM_GD_MAX_REACTIONS": _lib.GD_MAX_REACTIONS,
              "FEDM_MAX_TAGS": _lib.MAX_TAGS, "FEDM_GD_BAL_MAX_GROUPS": _lib.GD_BAL_MAX_GROUPS}
    size = 0
    for kind, decls in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        for decl in decls.split(","):
            count = 1
            for dim in re.findall(r"\[([^\]]+)\]", decl):
                count *= eval(dim, {}, consts)      # noqa: S307 - the header's own constant expressions
            size += count * (8 if kind == "double" else 4)
    assert size == C.sizeof(_lib.GdBalanceOut) == 880
    assert f"#define FEDM_GD_BAL_MAX_GROUPS {_lib.GD_BAL_MAX_GROUPS}" in text


def _stub_device(model):
    from oracle import gd as ogd
    o = ogd.GlowDischarge(DECK, 2, 2)
    calls = []
    dev = types.SimpleNamespace(model=model, cells=o.mesh.cells, coords=o.mesh.coords, nv=o.mesh.nv,
                                facet_tags=lambda: o.tags, dirichlet_vertices=lambda: np.concatenate([o.powered, o.grounded]),
                                balance_setup=lambda **kw: calls.append(kw), balance=lambda: "balance")
    return dev, o, calls


def test_discharge_balance_refuses_what_it_cannot_do():
    from fedm_amd import functions as ff
    from fedm_amd.cases import streamer
    from oracle import gd as ogd
    gd_model = oracle_model(ogd.GlowDischarge(DECK, 2, 2))
    dev, o, calls = _stub_device(streamer.model())
    with pytest.raises(ValueError, match="LMEA models only"):          # an LFA model
        ff.Discharge_balance(dev)
    with pytest.raises(ValueError, match="LMEA models only"):
        ff.Discharge_balance(types.SimpleNamespace(device=dev))
    dev.model = gd_model
    # tags 1, 2: the electrodes (Dirichlet); tag 3: the axis, whose two end vertices are electrode vertices
    with pytest.raises(ValueError, match="belongs to one group"):
        ff.Discharge_balance(dev, boundary_tags=(1, 3))
    with pytest.raises(ValueError, match="at most 8"):
        ff.Discharge_balance(dev, boundary_tags=(1, 2, 4, 1, 2, 4, 1, 2, 4))
    assert not calls
    # what is accepted reaches the device problem's set-up, and the callable is its balance()
    psi = o.mesh.coords[:, 1] / o.gap
    fn = ff.Discharge_balance(types.SimpleNamespace(device=dev), boundary_tags=(1, 2), weighting_potential=psi)
    assert fn() == "balance" and len(calls) == 1 and calls[0]["n_groups"] == 2
    z = o.mesh.coords[:, 1]
    assert np.array_equal(calls[0]["vertex_groups"], np.where(np.abs(z) < 1e-15, 1, np.where(np.abs(z - o.gap) < 1e-15, 2, 0)))
    assert calls[0]["weighting_potential"] is psi
