"""The numpy restatement of the LMEA field output (tests/gd_fields_reference.py) pinned without a GPU: on the balance's
restatement (for a planar model the plain measure is the balance's weight, so the load vectors sum to the balance's
totals), on closed forms, on the visibility of every addend at the device's bounds, and on deliberate faults; then the
names, the bindings and the facade's dispatch.  Every figure is printed before it is asserted.
"""
import ctypes as C
import math
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import balance_reference as bref  # noqa: E402
import gd_fields_reference as gfr  # noqa: E402
import lmea_models  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps
SUM_BOUND, POINT_BOUND, VISIBLE = 1e-12, 4 * EPS, 1e-4
# The radial components on the irregular mesh.  The states' field points along z; the radial parts of E, of a flux and of
# the current are the nodal noise, whose sign changes from cell to cell, and among the 700 vertices of the irregular mesh
# (valence 4 to 11) one vertex of deck-shape-permuted has flux_r:3 cancel to 2.05e-5 of its terms (the next lowest:
# flux_r:3 of two-ions-full 1.15e-4, current_r 1.0e-4); on the 3 x 3 and 10 x 10 meshes every kind stays above 1e-4
# (lowest 1.85e-4, flux_r:0 of e-only).  There the figure asserted is 1e-6: the device is held to 1e-12 of the same sum,
# so an addend as large as the value itself still misses that bound a million times over.
VISIBLE_RADIAL_IRREGULAR = 1e-6
# the cases of tests/test_gpu_gd_fields.py: (model, mesh, planar)
GPU_CASES = [("e-only", "3x3", False), ("e-only", "10x10", False), ("e-only", "10x10", True), ("ion-e", "3x3", False),
             ("ion-e", "10x10", False), ("deck-shape-permuted", "10x10", False), ("deck-shape-permuted", "irregular", False),
             ("two-ions-small", "10x10", False), ("two-ions-small", "10x10", True), ("two-ions-full", "10x10", False),
             ("two-ions-full", "irregular", False)]


def projected_names(md):
    """every projected request of a model"""
    ns, nr = int(md.n_species), int(md.n_reactions)
    return (["E_r", "E_z", "E_norm", "reduced_field", "collision_loss", "joule", "current_r", "current_z"]
            + [f"rate:{j}" for j in range(nr)] + [f"source:{s}" for s in range(1, ns)]
            + [f"flux_r:{c}" for c in range(ns)] + [f"flux_z:{c}" for c in range(ns)])


# ---- 1: the planar identity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two-ions-small", "e-only"])
def test_planar_load_vectors_sum_to_the_balance(name):
    c = lmea_models.case(name, "10x10", planar=True)
    g = c.mesh
    bal = bref.reference(c.md, g.coords, g.cells, g.tags, c.fields, c.U, c.Uo, c.Uo1, c.dt, c.dt_old, c.rules[0], c.rules[1])
    r = gfr.of_case(c)
    nr, ns = int(c.md.n_reactions), int(c.md.n_species)
    rates = [r.reference(c.U, f"rate:{j}") for j in range(nr)]
    pairs = [(f"rate:{j}", rates[j], bal["reaction"][j]) for j in range(nr)]
    pairs += [("joule", r.reference(c.U, "joule"), bal["joule"]), ("collision_loss", r.reference(c.U, "collision_loss"),
                                                                   bal["collision_loss"])]
    worst = 0.0
    for what, p, s in pairs:
        got = math.fsum(p.b.tolist())
        ratio = abs(got - s.value) / s.abs
        worst = max(worst, ratio)
        print(f"[gd fields] planar {name}: sum_v b_v({what}) {got:.6e} balance {s.value:.6e} |difference| / sum|terms| {ratio:.2e}",
              flush=True)
        assert ratio <= SUM_BOUND, (what, ratio)
    for s in range(1, ns):
        got = math.fsum(r.reference(c.U, f"source:{s}").b.tolist())
        comb = bref.combine(bal["reaction"], [float(bal["net"][j, s]) for j in range(nr)])
        ratio = abs(got - comb.value) / comb.abs if comb.abs > 0.0 else abs(got)
        print(f"[gd fields] planar {name}: sum_v b_v(source:{s}) {got:.6e} sum_j net R_j {comb.value:.6e} ratio {ratio:.2e}", flush=True)
        assert ratio <= SUM_BOUND, (s, ratio)


# ---- 2: closed forms ---------------------------------------------------------------------------------------------------
def test_closed_forms_on_a_uniform_state():
    c = lmea_models.case("ion-e", "3x3")
    md, g = c.md, c.mesh
    ns, nr, nv = int(md.n_species), int(md.n_reactions), g.nv
    ie, E0 = ns - 1, 2.5e3
    u = np.array([np.log(3.0) + 30.0, 31.0, 30.0])                      # energy, A+, e
    U = np.column_stack([np.full(nv, u[0]), np.full(nv, u[1]), np.full(nv, u[2]), -E0 * g.coords[:, 1]])
    mu, D, k = [0.0, 0.02, 0.3], [0.0, 0.05, 0.7], [1e-16, 3e-52, 2e-14]
    rows = [np.full(nv, v) for v in mu + D] + [np.zeros(nv)] * (2 * ns) + [np.full(nv, v) for v in k] + [np.zeros(nv)] * nr
    fields = np.stack(rows + [np.full(nv, 3.0), np.full(nv, 3.0), np.full(nv, u[ie])])
    assert fields.shape[0] == c.model.n_fields
    r = gfr.Restatement(md, g.coords, g.cells, fields, c.rules[0])
    n = np.exp(u)
    sign = [float(md.sign[i]) for i in range(ns)]
    flux = [0.0] + [sign[s] * mu[s] * E0 * n[s] for s in range(1, ns)]
    N0 = float(md.N0)
    expect = {"E_r": 0.0, "E_z": E0, "E_norm": E0, "reduced_field": 1e21 * E0 / N0, "joule": mu[ie] * n[ie] * E0 * E0,
              "current_z": gfr.ELEMENTARY_CHARGE * sum(sign[s] * flux[s] for s in range(1, ns)),
              "flux_z:0": sign[ie] * (5.0 / 3.0) * mu[ie] * E0 * n[0], "mean_energy": 3.0}
    for s in range(1, ns):
        expect[f"flux_z:{s}"] = flux[s]
        expect[f"flux_r:{s}"] = 0.0
    for j in range(nr):
        R = k[j]
        for i in range(ns):
            R *= (N0 if i == 0 else n[i]) ** int(md.power[j][i])
        expect[f"rate:{j}"] = R
    for name, want in expect.items():
        p = r.reference(U, name)
        got = p.b / p.m if isinstance(p, gfr.Projected) else p.value
        scale = abs(want) if want != 0.0 else (E0 if name == "E_r" else max(abs(f) for f in flux))
        err = float(np.abs(got - want).max()) / scale
        print(f"[gd fields] closed form {name}: expected {want:.6e}, worst relative error {err:.2e}", flush=True)
        assert err <= 1e-12, (name, err)


# ---- 3: every addend is visible at the device's bound -------------------------------------------------------------------
@pytest.mark.parametrize("name,mesh_name,planar", GPU_CASES)
def test_every_projected_kind_is_visible(name, mesh_name, planar):
    c = lmea_models.case(name, mesh_name, planar=planar)
    r = gfr.of_case(c)
    worst = {}
    for req in projected_names(c.md):
        p = r.reference(c.U, req)
        if not p.abs.any():
            assert not p.b.any()                                        # (a 'reaction' species' flux, a species no reaction makes)
            continue
        assert np.all(p.abs > 0.0), req
        worst[req] = float((np.abs(p.b) / p.abs).min())
    low = min(worst, key=worst.get)
    print(f"[gd fields] {name} {mesh_name}{' planar' if planar else ''}: min_v |b_v| / sum|terms|_v, worst {low} {worst[low]:.2e}; "
          + " ".join(f"{k} {v:.1e}" for k, v in worst.items()), flush=True)
    for req, v in worst.items():
        radial = req.split(":")[0] in ("E_r", "flux_r", "current_r")
        assert v >= (VISIBLE_RADIAL_IRREGULAR if radial and mesh_name == "irregular" else VISIBLE), (req, v)


# ---- 4: deliberate faults miss the device's bounds ----------------------------------------------------------------------
@pytest.mark.parametrize("fault,model,req", [
    ("the 5/3 left off the energy flux", "ion-e", "flux_z:0"),
    ("net taken for power", "ion-e", "source:1"),
    ("a sentinel loss taken literally", "deck-shape-permuted", "collision_loss"),
    ("mu_d * dme dropped", "two-ions-small", "joule"),
    ("the gas included in the charge", "ion-e", "charge")])
def test_a_deliberate_fault_misses_the_bound(fault, model, req):
    c = lmea_models.case(model, "10x10")
    md = c.md
    if req == "charge":                                                 # a sign for component 0, which the charge must not read
        md = type(c.md).from_buffer_copy(c.md)
        md.sign[0] = 1.0
    good, bad = gfr.of_case(c, md=md).reference(c.U, req), gfr.of_case(c, fault=fault, md=md).reference(c.U, req)
    if isinstance(good, gfr.Projected):
        ratio = float((np.abs(bad.b - good.b) / (SUM_BOUND * good.abs)).max())
    else:
        ratio = float((np.abs(bad.value - good.value) / (POINT_BOUND * good.abs)).max())
    print(f"[gd fields] fault '{fault}' in {req} of {model}: worst error / bound {ratio:.2e}", flush=True)
    assert ratio > 100.0


# ---- 5: names, bindings, the facade --------------------------------------------------------------------------------------
def test_names():
    from fedm_amd.field_output import GD_KINDS, parse_gd_request, parse_request
    names = ("gas", "A+", "e")
    P = lambda n: parse_gd_request(n, 3, 5, 25, names)                  # noqa: E731
    assert P("state:3") == (GD_KINDS["state"], 3) and P("density:e") == (GD_KINDS["density"], 2)
    assert P("density:0") == (GD_KINDS["density"], 0) and P("charge") == (GD_KINDS["charge"], 0)
    assert P("mean_energy") == (35, 0) and P("table:24") == (36, 24) and P("E_r") == (37, 0) and P("E_z") == (38, 0)
    assert P("E_norm") == (39, 0) and P("reduced_field") == (40, 0) and P("rate:4") == (41, 4)
    assert P("source:A+") == (42, 1) and P("collision_loss") == (43, 0) and P("joule") == (44, 0)
    assert P("flux_r:0") == (45, 0) and P("flux_z:e") == (46, 2) and P("current_r") == (47, 0) and P("current_z") == (48, 0)
    assert P(("joule",)) == (44, 0) and P((46, 1)) == (46, 1) and P(("flux_z", "e")) == (46, 2)
    for bad, match in (("state:4", "out of range"), ("density:3", "out of range"), ("table:25", "out of range"),
                       ("rate:5", "out of range"), ("source:0", "out of range"), ("source:gas", "out of range"),
                       ("rate:e", "neither an index"), ("flux_z", "needs an index"), ("joule:1", "takes no index"),
                       ("head", "unknown kind"), ((6, 0), "unknown kind")):
        with pytest.raises(ValueError, match=match):
            P(bad)
    assert parse_request("rate:0", 2, 3, 1) == (6, 0)                     # the LFA family's names are what they were
    assert set(GD_KINDS.values()) == set(range(32, 49))


def test_the_entry_points_are_bound_under_abi_10():
    import re
    from fedm_amd import _lib, field_output
    assert _lib.ABI_VERSION == 10
    assert {"fedm_gd_fields_setup", "fedm_gd_probe_setup", "fedm_gd_fields"} <= set(_lib.exported_symbols())
    text = (ROOT / "include" / "fedm_hip.h").read_text()
    assert "#define FEDM_ABI_VERSION 10" in text
    for name in ("fedm_gd_fields_setup", "fedm_gd_probe_setup", "fedm_gd_fields"):
        assert re.search(r"\bint " + name + r"\(fedm_ctx \*ctx", text), name
    defines = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define FEDM_GD_FIELD_(\w+) (\d+)", text)}
    assert defines == field_output.GD_KINDS
    lfa = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define FEDM_FIELD_(\w+) (\d+)", text)}
    assert not set(lfa.values()) & set(defines.values())                 # numbers of their own
    assert C.sizeof(_lib.FieldReq) == 8 and C.sizeof(_lib.FieldOpts) == 32


class _StubDevice:
    """What Field_output touches: the model and the three calls of each family"""

    def __init__(self, model):
        self.model, self.calls = model, []

    def _res(self, requests, probes):
        return types.SimpleNamespace(nodal=np.arange(len(requests) * 2.0).reshape(len(requests), 2), finite=True,
                                     probes=np.zeros((len(requests), 1)) if probes else None)

    def gd_fields_setup(self, consistent=False):
        self.calls.append(("gd_fields_setup", consistent))

    def gd_probe_setup(self, points):
        self.calls.append(("gd_probe_setup", len(points)))

    def gd_fields(self, requests, probes=False, **kw):
        self.calls.append(("gd_fields", tuple(requests), kw["t_out"], kw["t_old"], kw["t"], kw["projection"], probes))
        return self._res(requests, probes)

    def fields_setup(self, consistent=False):
        self.calls.append(("fields_setup", consistent))

    def probe_setup(self, points):
        self.calls.append(("probe_setup", len(points)))

    def fields(self, requests, probes=False, **kw):
        self.calls.append(("fields", tuple(requests)))
        return self._res(requests, probes)


def test_the_facade_dispatches_on_the_model():
    from fedm_amd import functions as ff
    dev = _StubDevice(lmea_models.model("ion-e"))
    out = ff.Field_output(types.SimpleNamespace(device=dev), ["mean_energy", "E_norm"], probes=[[2.5e-3, 1e-3]],
                          projection="consistent", species_names=("gas", "A+", "e"))
    assert dev.calls == [("gd_fields_setup", True), ("gd_probe_setup", 1)]
    got = out(0.3, 0.0, 1.0)                                            # blendable kinds take times
    assert dev.calls[-1] == ("gd_fields", ("mean_energy", "E_norm"), 0.3, 0.0, 1.0, "consistent", True)
    assert set(got) == {"mean_energy", "E_norm", "probes", "finite"} and got["finite"]
    step = ff.Field_output(dev, ["mean_energy", "joule", "table:3", "flux_z:e"])
    n = len(dev.calls)
    with pytest.raises(ValueError, match=r"joule, table:3, flux_z:e"):
        step(0.3, 0.0, 1.0)
    assert len(dev.calls) == n                                          # refused before the device is asked
    assert set(step()) == {"mean_energy", "joule", "table:3", "flux_z:e", "finite"}
    assert set(step(1.0, 0.0, 1.0)) == set(step())                      # t_out == t: the new state alone
    with pytest.raises(ValueError, match="projection"):
        ff.Field_output(dev, ["joule"], projection="exact")
    # an LFA model goes where it went
    lfa = _StubDevice(types.SimpleNamespace())
    ff.Field_output(lfa, ["E_norm"])(0.3, 0.0, 1.0)
    assert lfa.calls == [("fields_setup", False), ("fields", ("E_norm",))]
