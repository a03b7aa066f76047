"""tests/lmea_family_reference.py and tests/lmea_models.py held to what they are for (CPU only).

* The restatement against ``oracle.gd.GlowDischarge.residual_jacobian`` on the argon deck (the one model both know):
  deck and sentinel losses, quadrature degrees 4 and 6, the 10 x 10 crossed mesh at the state of ``perturbed_case``.  Both
  are float64 numpy of the same formulae; measured worst figures (per-component scale for F, row-max scale for J):
  F 4.3e-16, J 6.7e-16 -- asserted at 1e-12 and 1e-11.
* Visibility: at the states of tests/lmea_models.py every addend class a model has reaches, in some row of its component,
  at least 1e-3 of that component's scale -- the largest sum of |addends| over the component's rows, which is no smaller
  than the max |F| the device's error is measured on.  Measured: the least visible class of any model and mesh is at
  2.5e-3 (the thermal part of the energy row's wall term of two-ions-full on the 3 x 3 mesh).
* Faults: every perturbation that applies to a model moves F by more than 100 x 1e-11 or J by more than 100 x 1e-9 in
  the metrics of tests/lmea_checks.py, on the 10 x 10 mesh every model runs on the GPU.  Measured: the smallest move of
  F is 3.4e-3 (a kd row dropped), of J for the Jacobian-only fault 3.7e-2.
* The LDS arithmetic of the family: byte counts, and which models lose the table of exponentials.
* The complex-step Jacobian against central differences of the restatement's own residual, with both signs of
  Gamma_i . n and of sign mu E_n among the wall points.  Measured: 4.0e-10 of the row's scale.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lmea_family_reference as fam  # noqa: E402
import lmea_models as lm  # noqa: E402
import test_balance_reference as tb  # noqa: E402
from lmea_checks import gd_lds, jacobian_error, residual_error  # noqa: E402

F_BOUND, J_BOUND = 1e-11, 1e-9          # what tests/test_gpu_lmea_family.py holds the device to
VISIBLE, FAULT_FACTOR = 1e-3, 100.0


@pytest.mark.parametrize("degree", [4, 6])
@pytest.mark.parametrize("losses", ["deck", "sentinels"])
def test_restatement_matches_the_oracle_on_the_deck(losses, degree):
    c = tb.perturbed_case(losses, degree)
    o = c.o
    assert o.mesh.nc == 400 and len(o.wq) == (6 if degree == 4 else 12)
    dv = o.dirichlet_values(2e-12)
    F_o, J_o = o.residual_jacobian(c.U, c.Uo, c.Uo1, c.dt, c.dt_old, c.co, c.me_old, c.me, c.Uo[:, 3], dv)
    r = fam.residual_jacobian(tb.oracle_model(o, degree=degree).to_c(), o.mesh.coords, o.mesh.cells, o.tags, c.fields, c.U,
                              c.Uo, c.Uo1, c.dt, c.dt_old, o.dirichlet_dofs, dv, ((o.xq, o.wq), (o.tq, o.wt)))
    f_err, j_err = residual_error(r.F, F_o), jacobian_error(r.J, J_o)
    print(f"[family] restatement against the oracle, {losses}, degree {degree}: F {f_err:.2e} J {j_err:.2e}")
    assert f_err < 1e-12 and j_err < 1e-11
    # the restatement's pattern is the oracle's non-zeros
    nz = (abs(J_o) > 0).astype(np.int8)
    assert (nz - nz.multiply(r.pattern.astype(np.int8))).nnz == 0


def _configurations():
    for name in lm.MODELS:
        for mesh in lm.MESHES:
            if mesh == "irregular" and name not in lm.IRREGULAR_FOR:
                continue
            yield name, mesh, False
        if name in lm.PLANAR_TOO:
            yield name, "10x10", True


def _visibility(r, n_eq, dirichlet_dofs):
    """{(class, component): largest share of the component's scale over its rows}"""
    total = sum(r.classes.values()).reshape(-1, n_eq)
    scale = total.max(axis=0)
    free = np.abs(r.F)
    free[dirichlet_dofs] = 0.0
    assert np.all(scale * (1.0 + 1e-12) >= free.reshape(-1, n_eq).max(axis=0))
    out = {}
    for name, v in r.classes.items():
        v = v.reshape(-1, n_eq)
        for comp in range(n_eq):
            if v[:, comp].max() > 0.0:
                out[name, comp] = v[:, comp].max() / scale[comp]
    return out


def _expected_classes(m):
    """the classes a model must show, from its descriptor"""
    ns, ie = m.n_species, m.n_species - 1
    want = {("Poisson gradient part", ns)}
    for i in range(1, ns):
        if m.sign[i]:
            want.add((f"charge part of species {i}", ns))
    for c in range(ns):
        s = ie if c == 0 else c
        want.add(("time term", c))
        if m.eq_type[s] == fam.REACTION:
            continue
        drift = m.eq_type[s] == fam.DRIFT_DIFFUSION_REACTION
        want |= {("diffusion flux", c), ("wall thermal part", c)}
        if drift:
            want |= {("drift flux", c), ("wall drift part", c)}
        if not drift or m.grad_diffusion[s]:
            want.add(("grad-D flux", c))
        if s == ie and fam.ions(m):
            want.add(("wall emission part", c))
    want.add(("Joule heating", 0))
    for j in range(m.n_reactions):
        kind = fam.sentinel_kind(m.energy_loss[j])
        if kind:
            want.add((f"sentinel share {j}", 0))
        elif m.energy_loss[j]:
            want.add((f"reaction {j} share", 0))
        for c in range(1, ns):
            if m.net[j][c]:
                want.add((f"reaction {j} share", c))
    return want


@pytest.mark.parametrize("name,mesh,planar", list(_configurations()))
def test_every_addend_class_is_visible(name, mesh, planar):
    c = lm.case(name, mesh, planar)
    r = lm.restate(c, jacobian=False)
    vis = _visibility(r, c.model.n_eq, c.dirichlet_dofs)
    assert set(vis) == _expected_classes(r.model), set(vis) ^ _expected_classes(r.model)
    least = min(vis, key=vis.get)
    print(f"[family] {name} {mesh} {'planar' if planar else 'axisymmetric'}: {len(vis)} classes, the least visible "
          f"{least} at {vis[least]:.2e} of its component's scale")
    assert vis[least] >= VISIBLE, (least, vis[least])
    # what the scaling promises: me > 0, u_e away from 0
    assert c.fields[-3:-1].min() > 0.0 and c.U[:, c.model.n_species - 1].min() > 30.0
    # every row of the field table is non-zero and non-constant
    assert np.all(np.abs(c.fields).min(axis=1) > 0.0) and np.all(c.fields.max(axis=1) > c.fields.min(axis=1))
    # four tags, corner cells with two tagged facets on the 3 x 3 mesh
    assert set(np.unique(c.mesh.tags)) == {0, 1, 2, 3, 4}
    if mesh == "3x3":
        assert c.mesh.nc == 18 and ((c.mesh.tags > 0).sum(axis=1) == 2).any()


def test_the_table_of_applicable_perturbations():
    seen = set()
    for name in lm.MODELS:
        m = fam.plain_model(lm.model(name).to_c())
        applies = {p for p, spec in fam.PERTURBATIONS.items() if spec.applies(m)}
        assert applies == set(lm.APPLIES[name]), (name, applies ^ set(lm.APPLIES[name]))
        seen |= applies
    assert seen == set(fam.PERTURBATIONS) and len(fam.PERTURBATIONS) >= 13


@pytest.mark.parametrize("name", list(lm.MODELS))
def test_every_applicable_fault_misses_the_bounds_by_a_factor_of_100(name):
    c = lm.case(name, "10x10")
    base = lm.restate(c, classes=False)
    n_eq = c.model.n_eq
    for p in lm.APPLIES[name]:
        spec = fam.PERTURBATIONS[p]
        bad = lm.restate(c, perturbation=p, classes=False, jacobian=False)
        f_err = residual_error(bad.F, base.F, n_eq)
        j_err = None
        if spec.jacobian_only:
            assert np.array_equal(bad.F, base.F), p
        if spec.jacobian_only or f_err <= FAULT_FACTOR * F_BOUND:
            j_err = jacobian_error(lm.restate(c, perturbation=p, classes=False).J, base.J)
        print(f"[family] {name}: '{p}' moves F by {f_err:.2e}" + ("" if j_err is None else f", J by {j_err:.2e}"))
        assert (not spec.jacobian_only and f_err > FAULT_FACTOR * F_BOUND) or \
            (j_err is not None and j_err > FAULT_FACTOR * J_BOUND), p


def test_lds_arithmetic_of_the_family():
    """The staged bytes, the table's, and which side of 80 KiB: the two NEQ = 6 models sit on either side at degree 4,
    and the deck loses the table at degree 6."""
    small = gd_lds(6, 3, 6)
    assert (small.staged, small.table, small.exp_table) == (54528, 18432, True) and small.staged + small.table == 72960
    full = gd_lds(6, 16, 6)
    assert (full.staged, full.exp_table, full.launch) == (94464, False, 95496) and full.launch > 64 * 1024
    deck6 = gd_lds(5, 7, 12)
    assert (deck6.staged, deck6.table, deck6.exp_table) == (59136, 30720, False) and 59136 + 30720 > 81920
    assert [gd_lds(5, 7, n).launch for n in (3, 6)] == [67656, 75336]      # the deck at degrees 2 and 4, with the table
    for name, on in (("e-only", True), ("ion-e", True), ("deck-shape-permuted", True), ("two-ions-small", True),
                     ("two-ions-full", False)):
        gm = lm.model(name)
        assert gd_lds(gm.n_eq, gm.n_reactions, 6).exp_table is on, name
    assert [lm.model(n).n_eq for n in lm.MODELS] == [3, 4, 5, 6, 6]
    assert lm.model("two-ions-full").n_reactions == 16


def _both_signs(values):
    v = np.concatenate([np.ravel(a) for a in values])
    return (v > 0).any() and (v < 0).any()


@pytest.mark.parametrize("name", ["e-only", "ion-e"])
def test_complex_step_jacobian_against_central_differences(name):
    """Column by column on the 3 x 3 mesh, and along three random directions on the 10 x 10 mesh: relative step 1e-6,
    agreement 1e-6 of the row's scale.  The wall points see both signs of sign mu E_n -- and, where there is an ion,
    of Gamma_i . n: both branches of every |x| and Max(x, 0)."""
    for mesh in ("3x3", "10x10"):
        c = lm.case(name, mesh)
        r = lm.restate(c, classes=False)
        assert _both_signs(r.wall_signs["drift"]), mesh
        if name == "ion-e":
            assert _both_signs(r.wall_signs["ion"]), mesh
        n = c.U.size
        row_scale = np.maximum(abs(r.J).max(axis=1).toarray().ravel(), 1e-300)

        def F_at(u_flat):
            kw = dict(jacobian=False, classes=False)
            return fam.residual_jacobian(c.md, c.mesh.coords, c.mesh.cells, c.mesh.tags, c.fields, u_flat.reshape(c.U.shape),
                                         c.Uo, c.Uo1, c.dt, c.dt_old, c.dirichlet_dofs, c.dirichlet_vals, c.rules, **kw).F
        u = c.U.ravel().copy()
        worst = 0.0
        if mesh == "3x3":
            for k in range(n):
                d = np.zeros(n)
                d[k] = 1e-6 * abs(u[k])
                fd = (F_at(u + d) - F_at(u - d)) / (2.0 * d[k])
                worst = max(worst, (np.abs(fd - r.J[:, k].toarray().ravel()) / row_scale).max())
        else:
            rng = np.random.default_rng(3)
            for _ in range(3):
                v = rng.choice([-1.0, 1.0], n)
                d = 1e-6 * np.abs(u) * v
                fd = (F_at(u + d) - F_at(u - d)) / 2.0
                worst = max(worst, (np.abs(fd - r.J @ d) / (row_scale * 1e-6 * np.abs(u).max())).max())
        print(f"[family] {name} {mesh}: complex step against central differences {worst:.2e}")
        assert worst < 1e-6
