"""The per-step LMEA coefficient refresh of csrc/gdprep.hip, kernel by kernel, against the float64 numpy restatement of
tests/lmea_refresh_reference.py (itself held to the oracle by tests/test_lmea_refresh_reference.py): the coloured
right-hand side and the Jacobi-CG mass solve in both of its forms (one resident launch with counter barriers;
launch by launch with a replayed graph), the np.interp look-ups at their clamped ends, exact knots and degenerate
tables, the derived rows and the mean-energy bookkeeping, the failure path and the refusals of the set-up.

Meshes: the smallest at which a path changes -- 25 vertices (less than one slice of 64: 63 of the 64 waves of the
one-launch grid own no slice), 65 (one row in the second slice), 128 (two full slices), 8321 (131 slices, the first
grid of 9 workgroups), 33025 (517 slices, the 32-workgroup grid of the workload's size) and the refined Delaunay
mesh of test_gpu_unstructured.py (2468 vertices, a non-trivial vertex reordering, graded cells).

Tolerances and where they come from:
* reduced field: max |redE_dev - redE_LU| <= 1e-12 max |redE_LU|.  Jacobi-CG in float64 numpy, at the device's
  tolerance, ends 3e-16..2.1e-14 from LU on these meshes and potentials (test_lmea_refresh_reference.py); 1e-12 is
  50x that, for the device's other summation order and the extra iteration the launch-by-launch form may run.
  MEASURED on the MI355X (max |dev - LU| / max |LU|, ramp | steep potential):
      vertices   one launch             launch by launch
         25      1.2e-15 | 7.1e-16      9.2e-16 | 5.3e-16
         65      1.9e-14 | 3.8e-15      7.4e-15 | 1.4e-15
        128      1.9e-14 | 4.9e-15      5.5e-15 | 1.3e-15
       8321      1.8e-14 | 7.9e-15      5.4e-15 | 2.6e-15
      33025      1.6e-14 | 8.9e-15      5.5e-15 | 3.2e-15
       2468      1.5e-14 | 2.2e-15      5.0e-15 | 2.0e-15      (the refined mesh)
  The one-launch form stops where the numpy CG stops and lands where it lands (1.9e-14 at worst); the other form
  runs one iteration more, as its convergence test trails by one.
  A constant potential (-256 V) on the refined mesh, where the coordinate differences do not cancel exactly: max
  |redE| = 4.1e-12 Td in both forms, against a rounding bound of 9.4e-10 Td (and exactly 0 on the crossed meshes).
* look-ups: bitwise at clamped ends and exact knots; elsewhere |dev - ref| <= 2 eps (|fp_j| + |fp_j+1|) |scale|:
  the device may fuse slope * (x - xp_j) + fp_j into one rounding, which sits at most 0.83 eps (|fp_j| + |fp_j+1|)
  from np.interp on the deck's tables; unfused they are bit-equal.
  MEASURED: at worst 0.93 eps (|fp_j| + |fp_j+1|) |scale|, in both CG forms (the deck's tables and the two-entry ones).
* mean energy: |dev - exp(a)| <= (2 + |a|) eps exp(a), a = u_0 - u_e: half an ulp of a is |a| eps / 2 in exp's
  relative error, the rest is exp itself.  MEASURED: at worst 1.00 eps, 0.47 of the bound.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lmea_refresh_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps

MESHES = {
    "crossed 3x3": lambda: dict(nx=3, ny=3),
    "crossed 1x21": lambda: dict(nx=1, ny=21),
    "crossed 2x25": lambda: dict(nx=2, ny=25),
    "crossed 64x64": lambda: dict(nx=64, ny=64),
    "crossed 128x128": lambda: dict(nx=128, ny=128),
    "refined": lambda: dict(mesh=ref.refined()),
}
VERTICES = {"crossed 3x3": 25, "crossed 1x21": 65, "crossed 2x25": 128, "crossed 64x64": 8321,
            "crossed 128x128": 33025, "refined": 2468}
CG_FORMS = ["one launch", "launches"]


class _Cases:
    """One ``Case`` per mesh for the whole module (its multigrid set-up is the expensive part); the refresh
    pipeline is installed anew by every test, with its own tables and CG form."""

    def __init__(self):
        self.cases = {}

    def get(self, name):
        from fedm_amd.cases import glow_discharge as gdc
        if name not in self.cases:
            case = gdc.Case(device_pipeline=False, T_final=1.0, **MESHES[name]())
            assert case.mesh.num_vertices() == VERTICES[name]
            self.cases[name] = case
        return self.cases[name]

    def close(self):
        for case in self.cases.values():
            case.prob.close()


@pytest.fixture(scope="module")
def cases():
    c = _Cases()
    yield c
    c.close()


@pytest.fixture(scope="module")
def deck():
    d = ref.read_deck()
    return d, ref.deck_programs(d)


def _install(case, tables, programs, cg, monkeypatch):
    """FEDM_GD_CG is read by every gd_prep_setup."""
    monkeypatch.setenv("FEDM_GD_CG", "launches" if cg == "launches" else "one")
    case.prob.gd_prep_setup(tables, programs)


def _state(case, Phi, seed=3):
    """A state with the potential Phi; the other columns are random but plausible."""
    nv, n_eq = case.mesh.num_vertices(), case.prob.n_eq
    rng = np.random.default_rng(seed)
    U = rng.normal(0.0, 1.0, (nv, n_eq)) + 25.0
    U[:, n_eq - 1] = Phi
    Uo = rng.normal(0.0, 1.0, (nv, n_eq)) + 25.0
    return U, Uo, Uo + 0.1


def _random_fields(case, seed=4):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.5, 2.0, (case.prob.model.n_fields, case.mesh.num_vertices()))
    f[-2] = np.exp(rng.uniform(np.log(0.5), np.log(30.0), f.shape[1]))           # a mean energy inside the tables
    return f


def _step(case, fields, U, Uo, Uo1):
    prob = case.prob
    prob.set_gd_fields(fields)
    prob.set_state(U, Uo, Uo1)
    prob.gd_prep_step()
    return prob.get_gd_fields(), prob.get_gd_reduced_field()


def _lookup_check(dev_row, arg, table, scale, what):
    """np.interp's value at arg: bitwise at clamped ends and knots, 2 eps (|fp_j| + |fp_j+1|) |scale| elsewhere.
    Returns the worst distance in units of eps (|fp_j| + |fp_j+1|) |scale|."""
    xp, fp = (np.asarray(a, dtype=np.float64) for a in table)
    want = np.interp(arg, xp, fp) * scale
    exact = (arg <= xp[0]) | (arg >= xp[-1]) | np.isin(arg, xp)
    assert np.array_equal(dev_row[exact], want[exact]), f"{what}: clamped end or exact knot not bitwise np.interp's"
    if exact.all():
        return 0.0
    j = np.clip(np.searchsorted(xp, arg[~exact], side="right") - 1, 0, xp.size - 2)
    unit = EPS * (np.abs(fp[j]) + np.abs(fp[j + 1])) * abs(scale)
    err = np.abs(dev_row[~exact] - want[~exact])
    assert (err <= 2.0 * unit).all(), f"{what}: {np.max(err / np.maximum(unit, 1e-300)):.2f} units inside the table"
    return float(np.max(err / np.maximum(unit, 1e-300)))


def _check_rows(new, redE, fields, Uo, tables, programs, what):
    """Every row of a refresh result against the restatement's rules, the E/N look-ups at redE as read back."""
    n_eq = Uo.shape[1]
    me = fields[ref._row_of(programs, "me")]
    worst = 0.0
    for r, p in enumerate(programs):
        if p["kind"] in ("keep", "me"):
            assert np.array_equal(new[r], fields[r]), f"{what}: row {r} ({p['kind']}) changed"
        elif p["kind"] == "me_old":
            assert np.array_equal(new[r], me), f"{what}: mean_energy_old is not the previous mean energy"
        elif p["kind"] == "ue_old":
            assert np.array_equal(new[r], Uo[:, n_eq - 2]), f"{what}: u_e_old is not ln n_e of the previous state"
        elif p["kind"] == "table":
            arg = me if p.get("arg", "energy") == "energy" else redE
            worst = max(worst, _lookup_check(new[r], arg, tables[p["table"]], p.get("scale", 1.0), f"{what}: row {r}"))
    for r, p in enumerate(programs):
        if p["kind"] == "scaled_row":
            want = p["scale"] * new[p["src_row"]]                                    # one product, one rounding
            assert (np.abs(new[r] - want) <= EPS * np.abs(want)).all(), f"{what}: row {r} (scaled row)"
    return worst


# ---- the reduced field ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cg", CG_FORMS)
@pytest.mark.parametrize("name", list(MESHES))
def test_reduced_field_against_the_lu_projection(cases, deck, name, cg, monkeypatch):
    case = cases.get(name)
    d, (tables, programs) = deck
    assert ref.same_programs((tables, programs), ref.deck_programs(case))
    _install(case, tables, programs, cg, monkeypatch)
    m = case.mesh
    fields = _random_fields(case)
    for which in ("ramp", "steep"):
        U, Uo, Uo1 = _state(case, ref.potential(m.coords, which))
        new, redE = _step(case, fields, U, Uo, Uo1)
        want = ref.reduced_field(m.coords, m.cells, case.N0, U[:, -1])
        dist = np.abs(redE - want).max() / np.abs(want).max()
        print(f"reduced field, {name}, {cg}, {which}: {dist:.2e} of max |redE| from LU")
        assert dist <= 1e-12
        _check_rows(new, redE, fields, Uo, tables, programs, f"{name}/{cg}/{which}")


def _rounding_bound_of_a_constant(m, N0, value):
    """What the rounding of sum_a c (x_b - x_c) may leave of the reduced field of a constant potential c on a mesh
    whose coordinate differences do not cancel exactly.  A component of a cell's gradient numerator: the three
    differences round by eps / 2 each (their exact sum is zero), the three products by eps / 2 each, the two sums by
    eps / 2 of at most 2 |c| e each, e the cell's longest edge -- 5 eps |c| e in all, less where operations are fused;
    so f_cell <= 1e21 / N0 * sqrt(2) * 5 eps |c| e / |det|.  The projection of a cell-wise field bounded by F is bounded
    by F times the largest absolute row sum of M^-1 B (B: the cell-to-vertex load matrix |det| / 6), computed here."""
    import scipy.sparse as sp
    x = m.coords[m.cells]
    e = np.max([np.linalg.norm(x[:, i] - x[:, j], axis=1) for i, j in ((0, 1), (1, 2), (0, 2))], axis=0)
    det = np.abs(ref._geometry(m.coords, m.cells)[1])
    F = 1e21 / N0 * np.sqrt(2.0) * 5.0 * EPS * abs(value) * np.max(e / det)
    nc, nv = m.cells.shape[0], m.coords.shape[0]
    B = sp.coo_matrix((np.repeat(det / 6.0, 3), (m.cells.ravel(), np.repeat(np.arange(nc), 3))), shape=(nv, nc))
    spread = np.abs(np.linalg.solve(ref.mass_matrix(m.coords, m.cells).toarray(), B.toarray())).sum(axis=1).max()
    return 1.01 * spread * F


@pytest.mark.parametrize("cg", CG_FORMS)
@pytest.mark.parametrize("name", list(MESHES))
def test_a_potential_without_a_gradient_gives_exactly_zero(cases, deck, name, cg, monkeypatch):
    """The right-hand side is exactly zero and the CG returns x = 0 without an iteration (its rr0 == 0 path); every
    E/N row is then the first table entry times its scale, bitwise.  The constant is a power of two: its products
    with the coordinate differences are exact, fused or not, and on the crossed meshes the three differences of a cell
    cancel exactly (two of them are exact by Sterbenz's lemma, their sum rounds to the negative of the third) -- the
    restatement's own right-hand side says whether a mesh has that property.  The Delaunay mesh has not: there the
    constant must leave no more than its rounding, and the look-ups are held to np.interp at what it left."""
    case = cases.get(name)
    d, (tables, programs) = deck
    _install(case, tables, programs, cg, monkeypatch)
    m = case.mesh
    fields = _random_fields(case)
    cancels = not np.any(ref.reduced_field_rhs(m.coords, m.cells, case.N0, np.full(m.num_vertices(), -256.0)))
    assert cancels == (name != "refined")
    for value in (0.0, -256.0):
        U, Uo, Uo1 = _state(case, np.full(m.num_vertices(), value))
        new, redE = _step(case, fields, U, Uo, Uo1)
        if value == 0.0 or cancels:
            assert np.array_equal(redE, np.zeros_like(redE)), f"constant potential {value}"
            n_en = 0
            for r, p in enumerate(programs):
                if p["kind"] == "table" and p.get("arg") == "redfield":
                    assert np.array_equal(new[r], np.full_like(redE, tables[p["table"]][1][0] * p.get("scale", 1.0)))
                    n_en += 1
            assert n_en >= 1
        else:
            bound = _rounding_bound_of_a_constant(m, case.N0, value)
            print(f"constant potential {value} on {name}, {cg}: max |redE| = {np.abs(redE).max():.2e} Td, "
                  f"rounding bound {bound:.2e} Td")
            assert bound < 1e-6 and np.abs(redE).max() <= bound
        _check_rows(new, redE, fields, Uo, tables, programs, f"{name}/{cg}/constant {value}")


# ---- the look-ups ---------------------------------------------------------------------------------------------------
def _edge_tables(tables, programs):
    """The deck's programs with four of their 'keep' rows turned into look-ups of a two-entry and a one-entry table,
    by energy and by E/N."""
    tables = list(tables) + [(np.array([0.5, 50.0]), np.array([2.0, -7.0])), (np.array([3.0]), np.array([-1.25])),
                             (np.array([100.0, 3e4]), np.array([1e-3, 5e-3])), (np.array([40.0]), np.array([7.5]))]
    programs = [dict(p) for p in programs]
    keep = [r for r, p in enumerate(programs) if p["kind"] == "keep"]
    n = len(tables)
    for r, t, arg, scale in zip(keep, (n - 4, n - 3, n - 2, n - 1), ("energy", "energy", "redfield", "redfield"),
                                (1.0, 3.0, 1.0 / 3.0, 1.0)):
        programs[r] = dict(kind="table", table=t, arg=arg, scale=scale)
    return tables, programs


def _edge_energies(nv, xp, seed=5):
    """Log-uniform values past both ends of the table, every knot, its two neighbours in float64, the end knots."""
    rng = np.random.default_rng(seed)
    special = np.concatenate([xp, np.nextafter(xp, -np.inf), np.nextafter(xp, np.inf), [xp[0], xp[-1]]])
    assert special.size < nv
    me = np.exp(rng.uniform(np.log(1e-3), np.log(1e5), nv))
    me[rng.choice(nv, special.size, replace=False)] = special
    return me


@pytest.mark.parametrize("cg", CG_FORMS)
def test_look_ups_at_table_ends_knots_and_degenerate_tables(cases, deck, cg, monkeypatch):
    case = cases.get("crossed 64x64")
    d, (tables, programs) = deck
    tables, programs = _edge_tables(tables, programs)
    _install(case, tables, programs, cg, monkeypatch)
    m = case.mesh
    nv = m.num_vertices()
    xe = tables[1][0]                                            # the electron tables' energy axis
    assert xe[0] == 0.0353075 and xe[-1] == 22534.8 and all(np.array_equal(t[0], xe) for t in tables[1:15])
    fields = _random_fields(case)
    fields[-2] = _edge_energies(nv, xe)
    # the cathode fall within 5e-5 m: E/N from below zero (the projection overshoots) to past the last knot
    U, Uo, Uo1 = _state(case, ref.potential(m.coords, "steep", fall=5e-5))
    new, redE = _step(case, fields, U, Uo, Uo1)
    xr = tables[0][0]
    assert xr[0] == 0.0 and xr[-1] == 56497.2
    assert (redE < 0.0).sum() > 10 and (redE > xr[-1]).sum() > 10 and ((redE > 0) & (redE < xr[-1])).sum() > 1000
    want = ref.reduced_field(m.coords, m.cells, case.N0, U[:, -1])
    assert np.abs(redE - want).max() <= 1e-12 * np.abs(want).max()
    worst = _check_rows(new, redE, fields, Uo, tables, programs, f"look-ups/{cg}")
    print(f"look-ups, {cg}: worst {worst:.2f} eps (|fp_j| + |fp_j+1|) |scale| inside a table")
    # the degenerate tables took part
    kinds = [(p["kind"], p.get("table")) for p in programs]
    assert all(("table", t) in kinds for t in range(len(tables)))


def test_deck_programs_end_to_end_on_the_refined_mesh(cases, monkeypatch):
    """The programs ``Case._install_device_pipeline`` hands over, on the mesh with a vertex reordering."""
    case = cases.get("refined")
    prob, got = case.prob, {}
    setup = prob.gd_prep_setup
    monkeypatch.setenv("FEDM_GD_CG", "one")
    monkeypatch.setattr(prob, "gd_prep_setup", lambda t, p: (got.update(tables=t, programs=p), setup(t, p)))
    case._install_device_pipeline()
    monkeypatch.undo()
    tables, programs = got["tables"], got["programs"]
    assert ref.same_programs((tables, programs), ref.deck_programs(ref.read_deck()))
    m = case.mesh
    fields = _random_fields(case)
    fields[-2] = np.exp(np.random.default_rng(8).uniform(np.log(1e-2), np.log(1e5), m.num_vertices()))
    U, Uo, Uo1 = _state(case, ref.potential(m.coords, "steep"))
    new, redE = _step(case, fields, U, Uo, Uo1)
    want, want_redE = ref.refresh(m.coords, m.cells, case.N0, tables, programs, fields, U, Uo)
    assert np.abs(redE - want_redE).max() <= 1e-12 * np.abs(want_redE).max()
    _check_rows(new, redE, fields, Uo, tables, programs, "deck programs")
    # ... and against the restatement as a whole: an E/N row moves with redE's 1e-12 through its table's steepest slope
    def table_tol(p, moved):
        xp, fp = tables[p["table"]]
        slope = np.abs(np.diff(fp) / np.diff(xp)).max()
        return (slope * moved + 4.0 * EPS * np.abs(fp).max()) * abs(p.get("scale", 1.0))
    tol = [table_tol(p, 1e-12 * np.abs(want_redE).max() if p.get("arg") == "redfield" else 0.0)
           if p["kind"] == "table" else 0.0 for p in programs]
    for r, p in enumerate(programs):
        if p["kind"] == "scaled_row":
            tol[r] = abs(p["scale"]) * tol[p["src_row"]] + EPS * np.abs(want[r]).max()
    for r in range(len(programs)):
        assert (np.abs(new[r] - want[r]) <= tol[r]).all(), (r, programs[r])


# ---- bookkeeping ----------------------------------------------------------------------------------------------------
def test_mean_energy_update(cases, deck, monkeypatch):
    case = cases.get("crossed 64x64")
    d, (tables, programs) = deck
    _install(case, tables, programs, "one launch", monkeypatch)
    nv, n_eq = case.mesh.num_vertices(), case.prob.n_eq
    rng = np.random.default_rng(6)
    U = rng.normal(0.0, 1.0, (nv, n_eq)) + 25.0
    arg = rng.uniform(-40.0, 40.0, nv)
    arg[:4] = [-40.0, 40.0, 0.0, 1.0]
    U[:, 0] = U[:, n_eq - 2] + arg
    fields = _random_fields(case)
    case.prob.set_gd_fields(fields)
    case.prob.set_state(U, U, U)
    case.prob.gd_update_mean_energy()
    new = case.prob.get_gd_fields()
    a = U[:, 0] - U[:, n_eq - 2]
    want = ref.mean_energy(U)
    rel = np.abs(new[-2] - want) / want
    print(f"mean energy: worst {np.max(rel / EPS):.2f} eps, {np.max(rel / ((2.0 + np.abs(a)) * EPS)):.3f} of its bound")
    assert (rel <= (2.0 + np.abs(a)) * EPS).all()
    rows = np.ones(len(programs), dtype=bool)
    rows[-2] = False
    assert np.array_equal(new[rows], fields[rows])               # nothing else is touched


@pytest.mark.parametrize("cg", CG_FORMS)
def test_two_refreshes_with_a_mean_energy_update_in_between(cases, deck, cg, monkeypatch):
    """refresh, mean-energy update from the new state, shift, refresh: what two steps of the time loop do to the
    fields.  The second restated refresh starts from the mean energy as the device updated it (held to its own bound
    above), so that every look-up is judged on its own."""
    case = cases.get("refined")
    d, (tables, programs) = deck
    _install(case, tables, programs, cg, monkeypatch)
    m, prob = case.mesh, case.prob
    fields = _random_fields(case)
    U0, Uo0, Uo10 = _state(case, ref.potential(m.coords, "ramp"), seed=11)
    new1, redE1 = _step(case, fields, U0, Uo0, Uo10)
    want1, want_redE1 = ref.refresh(m.coords, m.cells, case.N0, tables, programs, fields, U0, Uo0)
    assert np.abs(redE1 - want_redE1).max() <= 1e-12 * np.abs(want_redE1).max()
    _check_rows(new1, redE1, fields, Uo0, tables, programs, "first refresh")
    # "the solve": a new state with another potential and another energy
    U1, _, _ = _state(case, ref.potential(m.coords, "steep", seed=12), seed=13)
    U1[:, 0] = U1[:, -2] + np.random.default_rng(14).uniform(-3.0, 9.0, m.num_vertices())
    prob.set_state(U1, None, None)
    prob.gd_update_mean_energy()
    after = prob.get_gd_fields()
    a = U1[:, 0] - U1[:, -2]
    assert (np.abs(after[-2] - ref.mean_energy(U1)) <= (2.0 + np.abs(a)) * EPS * ref.mean_energy(U1)).all()
    assert np.array_equal(after[:-2], new1[:-2]) and np.array_equal(after[-1], new1[-1])
    prob.shift_state()                                           # u_old <- u: the next step's previous state is U1
    prob.gd_prep_step()
    new2, redE2 = prob.get_gd_fields(), prob.get_gd_reduced_field()
    want2, want_redE2 = ref.refresh(m.coords, m.cells, case.N0, tables, programs, after, U1, U1)
    assert np.abs(redE2 - want_redE2).max() <= 1e-12 * np.abs(want_redE2).max()
    _check_rows(new2, redE2, after, U1, tables, programs, "second refresh")
    assert np.array_equal(new2[-3], after[-2]) and np.array_equal(new2[-3], want2[-3])
    assert np.array_equal(new2[-1], want2[-1])


# ---- failure and recovery -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cg", CG_FORMS)
def test_a_nan_in_the_potential_is_reported_and_leaves_the_fields_alone(cases, deck, cg, monkeypatch):
    case = cases.get("crossed 64x64")
    d, (tables, programs) = deck
    _install(case, tables, programs, cg, monkeypatch)
    m, prob = case.mesh, case.prob
    fields = _random_fields(case)
    U, Uo, Uo1 = _state(case, ref.potential(m.coords, "ramp"))
    bad = U.copy()
    bad[m.num_vertices() // 2, -1] = np.nan
    prob.set_gd_fields(fields)
    prob.set_state(bad, Uo, Uo1)
    with pytest.raises(RuntimeError, match="NaN or Inf"):
        prob.gd_prep_step()
    assert np.array_equal(prob.get_gd_fields(), fields)
    prob.set_state(U, Uo, Uo1)
    prob.gd_prep_step()
    new, redE = prob.get_gd_fields(), prob.get_gd_reduced_field()
    want = ref.reduced_field(m.coords, m.cells, case.N0, U[:, -1])
    assert np.abs(redE - want).max() <= 1e-12 * np.abs(want).max()
    _check_rows(new, redE, fields, Uo, tables, programs, f"after a failure/{cg}")


# ---- refusals -------------------------------------------------------------------------------------------------------
def _raw_setup(prob, tab_ptr, tab_x, tab_y, progs):
    """fedm_gd_prep_setup with the arrays as given (the binding's gd_prep_setup cannot build a wrong tab_ptr)."""
    import scipy.sparse as sp
    from fedm_amd import _lib, amg
    keep = []
    mass = amg._csr_struct(sp.identity(prob.nv, format="csr"), keep)
    ptr = np.ascontiguousarray(tab_ptr, dtype=np.int32)
    arr = (_lib.GdFieldProg * len(progs))()
    for r, (kind, table, arg, src_row, scale) in enumerate(progs):
        arr[r].kind, arr[r].table, arr[r].arg, arr[r].src_row, arr[r].scale = kind, table, arg, src_row, scale
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    x, y = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (tab_x, tab_y))
    rc = prob.lib.fedm_gd_prep_setup(prob._h, C.byref(mass), len(ptr) - 1, ptr.ctypes.data_as(C.POINTER(C.c_int32)),
                                     dp(x), dp(y), arr)
    return rc, _lib.last_error()


def test_set_up_refuses_what_np_interp_refuses(cases, deck, monkeypatch):
    """... on the host, before anything is allocated or launched: the installed pipeline, the fields and the
    pattern stay as they were.  (np.interp raises on an empty table; the kernel would have read xp[-1].)"""
    case = cases.get("crossed 2x25")
    d, (tables, programs) = deck
    _install(case, tables, programs, "one launch", monkeypatch)
    m, prob = case.mesh, case.prob
    fields = _random_fields(case)
    U, Uo, Uo1 = _state(case, ref.potential(m.coords, "ramp"))
    before, redE_before = _step(case, fields, U, Uo, Uo1)
    sizes = prob.sizes()
    nf = prob.model.n_fields
    keep = (0, 0, 0, 0, 1.0)
    x2, y2 = np.array([1.0, 2.0]), np.array([3.0, 4.0])
    look = lambda table=0, arg=0: [(1, table, arg, 0, 1.0)] + [keep] * (nf - 1)
    with pytest.raises(ValueError):
        np.interp(1.0, [], [])
    refused = {
        "tab_ptr does not start at 0": ([1, 3], np.zeros(3), np.zeros(3), look()),
        "tab_ptr decreases": ([0, 2, 1], x2, y2, look()),
        "a looked-up table has no entries": ([0, 2, 2], x2, y2, look(table=1)),
        "an empty table is the only one": ([0, 0], np.zeros(1), np.zeros(1), look()),
        "null tab_x": ([0, 2], None, y2, look()),
        "null tab_y": ([0, 2], x2, None, look()),
        "kind above its enum": ([0, 2], x2, y2, [(6, 0, 0, 0, 1.0)] + [keep] * (nf - 1)),
        "kind below its enum": ([0, 2], x2, y2, [(-1, 0, 0, 0, 1.0)] + [keep] * (nf - 1)),
        "arg outside its enum": ([0, 2], x2, y2, look(arg=2)),
    }
    for what, (ptr, x, y, progs) in refused.items():
        rc, message = _raw_setup(prob, ptr, x, y, progs)
        assert rc == -2 and message.startswith("fedm_gd_prep_setup"), (what, rc, message)
    with pytest.raises(RuntimeError, match="table without entries"):      # the same through the binding
        prob.gd_prep_setup(list(tables) + [(np.zeros(0), np.zeros(0))],
                           [dict(kind="table", table=len(tables), arg="energy")] + list(programs[1:]))
    # nothing changed: the pattern, the fields, and the pipeline installed before -- its step repeats bit by bit
    assert prob.sizes() == sizes
    assert np.array_equal(prob.get_gd_fields(), before)
    again, redE_again = _step(case, fields, U, Uo, Uo1)
    assert np.array_equal(again, before) and np.array_equal(redE_again, redE_before)
    # an empty table that no program looks up is nobody's np.interp: accepted; so are no entries at all with null arrays
    rc, message = _raw_setup(prob, [0, 2, 2], x2, y2, look(table=0))
    assert rc == 0, message
    rc, message = _raw_setup(prob, [0, 0], None, None, [keep] * nf)
    assert rc == 0, message
    prob.gd_prep_step()                                  # (identity mass matrix, nothing but 'keep' rows)
    assert np.array_equal(prob.get_gd_fields(), before)
