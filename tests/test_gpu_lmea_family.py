"""The LMEA assembly (csrc/gd.hip) and balance (csrc/gd_balance.hip) across their model family, against the numpy
restatement of tests/lmea_family_reference.py at the models, meshes and states of tests/lmea_models.py.

What the argon deck cannot show and these do: NEQ = 3, 4 and 6 (workgroups of 2, 3 and 5 waves, the LDS carve-up for
other field counts, the gathers at other NEQ); the element kernel without its table of exponentials (two-ions-full, and
the deck at quadrature degree 6); grad_diffusion on an ion and off on the electrons; two ions, one negative, in the
emission sum; a reaction-type species and a diffusion-reaction species at other indices; reaction powers of 4, an electron
power of 2, a gas power of 2; four tags with distinct reflection rows (ref = 0 and ref = 1 among them) and one without
emission; cells with two tagged facets; mu_d, D_d of the heavy species and kd of every reaction non-zero.

Bounds: F 1e-11 of its component's scale and J 1e-9 of its row's largest entry (tests/lmea_checks.py) -- what the same
kernels meet against the oracle on the deck.  tests/test_lmea_family_reference.py shows on the CPU that every addend class
is visible at these bounds and that every deliberate fault of the restatement misses them by more than a factor of 100.
The restatement's F and J are computed once per (model, mesh, geometry) and shared by the variants.
Every figure is printed before it is asserted.
"""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import balance_reference as bref  # noqa: E402
import lmea_family_reference as fam  # noqa: E402
import lmea_models as lm  # noqa: E402
import test_balance_reference as tb  # noqa: E402
from lmea_checks import gd_lds, jacobian_error, residual_error  # noqa: E402

pytestmark = pytest.mark.gpu
F_BOUND, J_BOUND = 1e-11, 1e-9
LAUNCHED = {"0": "lmea/dual-number colours", "2": "lmea/atomics", "4": "lmea/element buffer, cell order",
            "3": "lmea/element buffer, destination order",
            "5": "lmea/element buffer, destination order, columns side by side"}
# what a model's name does not say, for the test ids
FEATURES = {
    "e-only": "neq3-no-ion-empty-emission-sum",
    "ion-e": "neq4-ion-grad_diffusion-on-electrons-off-electron-power-2-gas-power-2",
    "deck-shape-permuted": "neq5-negative-ion-reaction-type-at-index-2-power-4-sentinels",
    "two-ions-small": "neq6-second-ion-negative-ion-diffusion-reaction-at-index-1-exp-table",
    "two-ions-full": "neq6-16-reactions-diffusion-reaction-at-index-2-no-exp-table-lds-grant",
}
MESH_FEATURES = {"3x3": "3x3-one-workgroup-two-tagged-facets", "10x10": "10x10-seven-workgroups", "irregular": "irregular"}
EXP_TABLE = {"e-only": True, "ion-e": True, "deck-shape-permuted": True, "two-ions-small": True, "two-ions-full": False}
_RESTATED = {}


def _restated(name, mesh, planar):
    key = (name, mesh, planar)
    if key not in _RESTATED:
        r = lm.restate(lm.case(name, mesh, planar), classes=False)
        r.F.setflags(write=False)
        _RESTATED[key] = r
    return _RESTATED[key]


def _problem(c, model=None):
    from fedm_amd.device import DeviceProblem
    prob = DeviceProblem(c.mesh.coords, c.mesh.cells, c.model if model is None else model, facet_tags=c.mesh.tags,
                         dirichlet_dofs=c.dirichlet_dofs, dirichlet_vals=c.dirichlet_vals, reorder=True)
    prob.set_gd_fields(c.fields)
    prob.set_state(c.U, c.Uo, c.Uo1)
    prob.set_step(c.dt, c.dt_old)
    return prob


def _assembly_cases():
    for name in lm.MODELS:
        neq6 = name.startswith("two-ions")
        configs = [(mesh, False) for mesh in lm.MESHES if mesh != "irregular" or name in lm.IRREGULAR_FOR]
        if name in lm.PLANAR_TOO:
            configs.append(("10x10", True))
        for mesh, planar in configs:
            runs = [("5", None, None), ("0", None, None)]
            if mesh == "10x10":
                runs += [("3", None, None), ("4", None, None), ("2", None, None)]
            if neq6:
                runs.append(("5", None, "positions"))
            if name == "deck-shape-permuted":
                runs.append(("5", "two", None))
            for hand, waves, gather in runs:
                ident = "-".join([FEATURES[name], MESH_FEATURES[mesh], "planar" if planar else "axisymmetric", f"hand{hand}"]
                                 + ([f"waves-{waves}"] if waves else []) + ([f"gather-{gather}"] if gather else []))
                yield pytest.param(name, mesh, planar, hand, waves, gather, id=ident)


@pytest.mark.parametrize("name,mesh,planar,hand,waves,gather", list(_assembly_cases()))
def test_assembly_with_four_tags_ref_0_ref_1_gamma_0_and_energy_dependent_heavy_coefficients(name, mesh, planar, hand, waves,
                                                                                            gather, monkeypatch):
    """F of the residual-only assembly, F and J of the F + J assembly, the launch record and the pattern, for one model,
    mesh and kernel variant.  Every model has four tags with distinct ref rows (ref = 0 and ref = 1 among them) and one
    gamma = 0, and non-zero mu_d, D_d and kd rows for every species and reaction."""
    monkeypatch.setenv("FEDM_GD_HAND", hand)
    monkeypatch.setenv("FEDM_GD_WAVES", waves or "auto")
    monkeypatch.setenv("FEDM_GD_GATHER", gather or "rows")
    c = lm.case(name, mesh, planar)
    ref = _restated(name, mesh, planar)
    neq, nc = c.model.n_eq, c.mesh.nc
    lds = gd_lds(neq, c.model.n_reactions, len(c.rules[0][1]))
    assert lds.exp_table is EXP_TABLE[name]
    if name == "two-ions-small":
        assert lds.staged + lds.table == 72960
    if name == "two-ions-full":
        assert (lds.staged, lds.launch) == (94464, 95496) and lds.launch > 64 * 1024
    prob = _problem(c)
    try:
        F_gpu, _ = prob.residual()
        f_err = residual_error(F_gpu, ref.F, neq)
        prob.jacobian()
        J_gpu = prob.jacobian_csr()
        j_err = jacobian_error(J_gpu, ref.J)
        fj_err = residual_error(prob.residual_vector(), ref.F, neq)
        rec = prob.launched_assembly()
        n_colours = prob.sizes()["n_colours"]
    finally:
        prob.close()
    print(f"[family] {name} {mesh} {'planar' if planar else 'axisymmetric'} hand {hand} waves {waves} gather {gather}: "
          f"F {f_err:.2e}, F of F + J {fj_err:.2e}, J {j_err:.2e}; LDS {lds.launch} bytes, table {lds.exp_table}; {rec}",
          flush=True)
    assert f_err < F_BOUND and fj_err < F_BOUND
    assert j_err < J_BOUND
    for what in ("residual", "jacobian"):
        assert rec[what]["variant"] == LAUNCHED[hand], (what, rec)
        assert rec[what]["launches"] == (n_colours if hand == "0" else 1), (what, rec)
        if hand != "0":
            two_waves = what == "jacobian" and hand == "5" and waves == "two" and neq == 5
            assert rec[what]["threads"] == (128 if two_waves else 64 * (neq - 1)), (what, rec)
            assert rec[what]["workgroups"] == -(-nc // 64), (what, rec)
    if hand != "0":
        # the same pattern: every position of the restatement is stored, and nothing outside it holds a value (the
        # restatement's pattern is structural -- coupled fields at vertices that share a cell -- so an entry that rounds
        # to something where two edges are perpendicular is inside it)
        stored = J_gpu.copy()
        stored.data[:] = 1.0
        pattern = ref.pattern.astype(np.float64)
        assert (pattern - pattern.multiply(stored)).nnz == 0
        nz = (abs(J_gpu) > 0).astype(np.float64)
        assert (nz - nz.multiply(pattern)).nnz == 0


def test_deck_degree6_without_the_exp_table_after_a_degree4_context():
    """The argon deck at quadrature degree 6 (12 points): staged data and table pass 80 KiB (59 136 + 30 720), so the
    production model runs without the table of exponentials -- in the same process after a degree-4 context, so the LDS
    grant grows a second time.  Held to the oracle with its rules at the same degree, and to the restatement."""
    import test_gpu_glow_discharge as tg
    from fedm_amd import quadrature
    from fedm_amd.cases import glow_discharge as gdc
    needs = []
    for degree in (4, 6):
        case = gdc.Case(nx=10, ny=10, device_pipeline=False, quadrature_degree=degree)
        ref = tg._reference(case, degree=degree)
        prob = tg._upload(case, ref)
        lds = gd_lds(5, prob.model.n_reactions, len(quadrature.triangle(degree)[1]))
        needs.append(lds)
        try:
            F_gpu, _ = prob.residual()
            prob.jacobian()
            J_gpu, FJ_gpu = prob.jacobian_csr(), prob.residual_vector()
            rec = prob.launched_assembly()
        finally:
            prob.close()
        f_err, fj_err, j_err = residual_error(F_gpu, ref["F"]), residual_error(FJ_gpu, ref["F"]), jacobian_error(J_gpu, ref["J"])
        print(f"[family] deck degree {degree}: LDS {lds}; against the oracle F {f_err:.2e}, F of F + J {fj_err:.2e}, "
              f"J {j_err:.2e}", flush=True)
        assert f_err < F_BOUND and fj_err < F_BOUND and j_err < J_BOUND, degree
        assert rec["jacobian"]["variant"] == LAUNCHED["5"] and rec["jacobian"]["threads"] == 256
        if degree == 6:
            c = tb.perturbed_case("deck", 6)
            o = c.o
            assert np.array_equal(c.U, ref["U"]) and np.array_equal(c.Uo, ref["Uo"])
            r = fam.residual_jacobian(tb.oracle_model(o, degree=6).to_c(), o.mesh.coords, o.mesh.cells, o.tags, c.fields, c.U,
                                      c.Uo, c.Uo1, c.dt, c.dt_old, o.dirichlet_dofs, o.dirichlet_values(ref["t"]),
                                      ((o.xq, o.wq), (o.tq, o.wt)), classes=False)
            f_err, j_err = residual_error(F_gpu, r.F), jacobian_error(J_gpu, r.J)
            print(f"[family] deck degree 6 against the restatement: F {f_err:.2e}, J {j_err:.2e}", flush=True)
            assert f_err < F_BOUND and j_err < J_BOUND
    assert needs[0].exp_table and needs[0].launch == 75336
    assert (needs[1].staged, needs[1].table, needs[1].exp_table) == (59136, 30720, False)
    assert needs[1].staged + needs[1].table > 81920


@pytest.mark.parametrize("hand", ["5", "3"])
def test_neq6_gathers_per_position_and_per_row_agree_bit_for_bit(hand, monkeypatch):
    """two-ions-full: the element buffer summed into the matrix by a thread per stored position and by a thread per
    (position, equation row) -- the same bytes of F and J at NEQ = 6."""
    monkeypatch.setenv("FEDM_GD_HAND", hand)
    c = lm.case("two-ions-full", "10x10")
    out = {}
    for gather in ("positions", "rows"):
        monkeypatch.setenv("FEDM_GD_GATHER", gather)
        prob = _problem(c)
        try:
            F_gpu, _ = prob.residual()
            prob.jacobian()
            assert prob.launched_assembly()["jacobian"]["variant"] == LAUNCHED[hand]
            out[gather] = (F_gpu, prob.residual_vector(), prob.jacobian_csr())
        finally:
            prob.close()
    Jp, Jr = out["positions"][2], out["rows"][2]
    assert np.array_equal(out["positions"][0], out["rows"][0]) and np.array_equal(out["positions"][1], out["rows"][1])
    assert np.array_equal(Jp.indptr, Jr.indptr) and np.array_equal(Jp.indices, Jr.indices)
    assert Jp.data.tobytes() == Jr.data.tobytes() and np.abs(Jp.data).max() > 0.0


def _psi(c):
    return c.mesh.coords[:, 1] / c.mesh.L + 0.2 * ((c.mesh.coords[:, 0] - lm.R0) / c.mesh.L) ** 2


@pytest.mark.parametrize("name,planar", [("ion-e", False), ("two-ions-small", False), ("two-ions-small", True),
                                         ("two-ions-full", False)],
                         ids=["ion-e", "two-ions-small-axisymmetric", "two-ions-small-planar", "two-ions-full"])
def test_balance_with_two_ions_and_four_distinct_tags(name, planar):
    """fedm_gd_balance against tests/balance_reference.reference at that file's bound (1e-12 of sum |terms|), and the
    identity rate_of_change - source + walls = the sum of the device's own residual rows at 1e-11.  With two ions the
    Ion_flux of a tag is a sum the deck cannot tell from its single addend; with four distinct tags no wall entry can
    stand in for another."""
    import test_gpu_balance as tgb
    c = lm.case(name, "10x10", planar)
    group = np.zeros(c.mesh.nv, dtype=np.int8)
    group[c.mesh.bottom], group[c.mesh.top] = 1, 2
    psi = _psi(c)
    args = (c.mesh.coords, c.mesh.cells, c.mesh.tags, c.fields, c.U, c.Uo, c.Uo1, c.dt, c.dt_old, c.rules[0], c.rules[1])
    ref = bref.reference(c.md, *args, psi=psi, group=group, n_groups=2)
    prob = _problem(c)
    try:
        prob.balance_setup(weighting_potential=psi, vertex_groups=group, n_groups=2)
        b = prob.balance()
        what = f"{name} {'planar' if planar else 'axisymmetric'}"
        tgb._check_sums(what, b, ref)
        tgb._check_identity(what, prob, b, ref)
    finally:
        prob.close()
    ns = c.model.n_species
    m = fam.plain_model(c.md)
    # the entries are told apart by far more than the bound: every tag's wall entry of a species with a flux differs
    # from every other tag's, and leaving the second ion out of Ion_flux would move it
    for comp in range(ns):
        s = ns - 1 if comp == 0 else comp
        if m.eq_type[s] == fam.REACTION:
            continue
        w = [ref["wall"][t][comp] for t in range(4)]
        for t in range(4):
            if m.ref[t][s] == 1.0 and not (s == ns - 1 and fam.ions(m) and m.gamma[t]):
                assert b.wall[t, comp] == 0.0           # everything reflected, nothing emitted: exactly nothing
            else:
                assert abs(b.wall[t, comp]) > 0.0
            for t2 in range(t):
                assert abs(w[t].value - w[t2].value) > 1e3 * tgb.SUM_BOUND * max(w[t].abs, w[t2].abs), (comp, t, t2)
    if len(fam.ions(m)) > 1:
        # on the side walls (tags 3 and 4: the field's normal component changes sign along them) both ions arrive:
        # Ion_flux is a sum of two addends there, and leaving either ion out would move it; an electrode sees the ions
        # of one sign only
        for drop in (0, 1):
            one_ion = fam.plain_model(c.md)
            one_ion.is_ion[fam.ions(one_ion)[drop]] = 0
            one = bref.reference(one_ion, *args)
            moved = [abs(one["ion_flux"][t].value - ref["ion_flux"][t].value) / ref["ion_flux"][t].abs for t in range(4)]
            print(f"[family] {what}: Ion_flux {b.ion_flux}; without ion {drop + 1} it moves by {moved} of sum |terms|", flush=True)
            assert moved[2] > 1e3 * tgb.SUM_BOUND and moved[3] > 1e3 * tgb.SUM_BOUND
            assert sum(v > 1e3 * tgb.SUM_BOUND for v in moved) >= 3
    assert math.isfinite(b.joule) and b.finite


def test_refusals_at_creation_and_a_context_afterwards_works(monkeypatch):
    """A power of 16, one or six species, 17 reactions and a sentinel loss without mean_energy_form: each refused with a
    message when the context is created -- by the binding where it checks, and by fedm_ctx_create_gd for a descriptor
    that reaches it -- and the next context assembles as if nothing had happened."""
    import dataclasses
    from fedm_amd.device import GdModel
    c = lm.case("ion-e", "3x3")

    def forged(change):
        """a model whose descriptor is changed after the binding's own checks"""
        class Forged(GdModel):
            def to_c(self):
                md = super().to_c()
                change(md)
                return md
        return Forged(**dataclasses.asdict(c.model))

    def set_(field, value):
        return lambda md: setattr(md, field, value)

    def power16(md):
        md.power[1][2] = 16
    fields = dataclasses.asdict(c.model)
    bad_power = [list(r) for r in c.model.power]
    bad_power[1][2] = 16
    refused = [
        ("a power of 16", GdModel(**{**fields, "power": bad_power}), RuntimeError, "powers must be between 0 and 15"),
        ("a power of 16, forged", forged(power16), RuntimeError, "powers must be between 0 and 15"),
        ("one species", forged(set_("n_species", 1)), RuntimeError, "unsupported LMEA model descriptor"),
        ("six species", forged(set_("n_species", 6)), RuntimeError, "unsupported LMEA model descriptor"),
        ("17 reactions", forged(set_("n_reactions", 17)), RuntimeError, "unsupported LMEA model descriptor"),
        ("a sentinel loss without mean_energy_form", GdModel(**{**fields, "energy_loss": [15.76, lm.S1, 2.5]}), ValueError,
         "need mean_energy_form"),
    ]
    for what, model, error, message in refused:
        with pytest.raises(error, match=message):
            _problem(c, model)
    # the binding's own refusals of what it cannot write into the descriptor
    six = lm.model("two-ions-small")
    with pytest.raises(ValueError, match="too large"):
        dataclasses.replace(six, n_species=6, eq_type=list(six.eq_type) + [lm.DD], grad_diffusion=list(six.grad_diffusion) + [0],
                            is_ion=list(six.is_ion) + [0], sign=list(six.sign) + [0.0], vth=list(six.vth) + [0.0]).to_c()
    with pytest.raises(ValueError, match="too large"):
        dataclasses.replace(c.model, power=[c.model.power[0]] * 17, net=[c.model.net[0]] * 17, energy_loss=[1.0] * 17).to_c()
    ref = _restated("ion-e", "3x3", False)
    prob = _problem(c)
    try:
        F_gpu, _ = prob.residual()
        prob.jacobian()
        f_err, j_err = residual_error(F_gpu, ref.F, 4), jacobian_error(prob.jacobian_csr(), ref.J)
    finally:
        prob.close()
    print(f"[family] after the refusals: F {f_err:.2e}, J {j_err:.2e}", flush=True)
    assert f_err < F_BOUND and j_err < J_BOUND
