"""Photoionisation on the device (csrc/photo.hip, DeviceProblem.photo_update) against the numpy / scipy restatement of
tests/photoionization_reference.py, which tests/test_photoionization_reference.py pins on a manufactured solution.

Meshes: (a) tensor 12 x 17 cells on the streamer box -- 234 vertices, four 64-vertex slices with the last partly
padding, not square; (b) a graded Delaunay mesh of the box with a few hundred vertices whose device numbering moves
more than half of them.  Models: the benchmark deck's closed forms and their tabulated twin
(tests/tabulated_reference.py), axisymmetric and not.  States: the oracle's initial state with the perturbations of
test_gpu_parity.py, u_new != u_old.  Terms: kappa = 0.1, 1, 10 over the mean edge length (stiffness-dominated, mixed,
mass-dominated) with three different c_m.

Bounds.  Load vector: 1e-11 of its largest entry, the bound test_gpu_parity.py holds F to.  Solves at rtol = 1e-10:
true residual of the restated operator at the device's y at most 2 rtol |b| (the factor 2 for the drift of the
recurrence's residual from the true one), error against spsolve at most 2 cond_2(A_ff) rtol |y_ref| with the condition
number of the free-free block from numpy.linalg.eigvalsh (|e| <= |A^-1| |r|, |b| <= |A| |y|).  Table: 4 eps.  Assembly
with the table against the same table set by hand: bitwise under the global colouring, the assembly that is bitwise
reproducible (the LDS-patch kernels add with LDS atomics and differ in the last bits between two runs of ONE problem:
see test_assembly_uses_the_table); against the oracle, under both: 1e-11 / 1e-10 as in test_gpu_unstructured.py.  One
BDF step against oracle.newton: the Newton count and 1e-9 per component, as test_streamer_newton_step.

MEASURED on the MI355X: load vector 1.4e-15 .. 9.3e-15 of its largest entry; true residuals 1.7e-11 .. 9.9e-11 of |b|
(bound 2e-10); errors against spsolve 4.8e-13 .. 6.0e-10 (bounds 9.2e-10 .. 3.2e-6, condition numbers 4.6 .. 16 057);
CG iterations per term with hierarchies 15-18 / 12-16 / 10-11, with Jacobi alone 67-78 / 34-49 / 17-19; F and J
against the oracle at most 1.6e-13 and 1.6e-14; the time step on the eight cases: Newton counts 2 = 2 (tensor mesh, four
cases), 3 = 3, 4 = 4, 3 = 3 and 3 against 4 (the case whose count is not compared, see test_a_time_step), states within
2.4e-14.  Every test runs on all eight cases; test_other_species_counts adds a one-species model without a Poisson
row and a three-species model with one.

The time-step test runs with efficiency 1.0: with the oracle alone (CPU), one step of 5e-12 s from the initial state
with and without the restated table differs in the ion component (relative to its largest entry) by 1.05e-7 on the
tensor mesh and 5.2e-8 on the Delaunay mesh at efficiency 0.01, by 1.05e-6 and 5.2e-7 at 0.1 -- not above the 1e-6
the comparison needs to see the table on both -- and by 1.05e-5 and 5.2e-6 at 1.0.
"""
import dataclasses
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, str(Path(__file__).resolve().parent))
import photoionization_reference as pr  # noqa: E402
import tabulated_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
RTOL = 1e-10
EFFICIENCY = 0.05
C_TERMS = (2.0e4, 1.5e6, 0.8e8)          # [1/m^2]: with kappa^2 ~ 1e4, 1e6, 1e8 every term weighs in
ZERO_TAGS = (1, 2)                        # the two electrodes
CASES = [(m, c, a) for m in ("tensor", "delaunay") for c in ("closed", "tabulated") for a in (True, False)]
IDS = [f"{m}-{c}-{'axi' if a else 'plane'}" for m, c, a in CASES]


def _mesh(name):
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh, rectangle_right
    if name == "tensor":
        m = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, 12, 17)
        assert m.nv == 234
        return m
    from fedm_amd import meshgen
    size = meshgen.box_distance_size((0.0, 1.5e-3, 7e-3, 11e-3), 3e-4, 0.6, 3e-3)
    g = meshgen.refined_rectangle(ost.BOX, ost.BOX, size, 3e-4, n_levels=3)
    assert 200 <= g.coords.shape[0] <= 700
    return OMesh(g.coords, g.cells)


def _models(mesh, coefficients, axisymmetric):
    """(oracle model, device Model without photoionisation) of one case."""
    from oracle import streamer as ost
    from fedm_amd.cases import streamer
    if coefficients == "closed":
        om, dm = ost.build(mesh), streamer.model()
    else:
        plain = ost.build(mesh)
        _, _, Em = plain.cell_fields(pr.perturbed(ost.initial_state(plain), 21))
        x = tr.quantile_knots(Em)
        om, dm = tr.oracle_streamer(mesh, x), tr.device_streamer_model(x)
    if not axisymmetric:
        om.axisymmetric = False
        om._geometry()
        dm = dataclasses.replace(dm, axisymmetric=False)
    return om, dm


class Case:
    """One (mesh, coefficients, geometry): the oracle model, the states, the restated update, and device problems made
    on demand (closed by the fixture)."""

    def __init__(self, mesh_name, coefficients, axisymmetric, efficiency=EFFICIENCY):
        from oracle import streamer as ost
        from fedm_amd.device import Photoionization
        self.mesh = _mesh(mesh_name)
        self.mesh_name = mesh_name
        self.om, self.dm = _models(self.mesh, coefficients, axisymmetric)
        self.U0 = ost.initial_state(self.om)
        self.U_old, self.U_new = pr.perturbed(self.U0, 21), pr.perturbed(self.U0, 22)
        h = pr.mean_edge_length(self.mesh.coords, self.mesh.cells)
        self.kappa = [0.1 / h, 1.0 / h, 10.0 / h]
        self.photo = Photoionization(reactions=[0], efficiency=efficiency, c=list(C_TERMS), kappa=self.kappa,
                                     targets=[0, 1], zero_tags=list(ZERO_TAGS), rtol=RTOL, max_it=2000,
                                     multigrid=True, max_coarse=40)
        self.ref = pr.reference(self.om, self.U_old, [0], efficiency, C_TERMS, self.kappa, ZERO_TAGS)
        self._open = []

    def problem(self, photo="default", **change):
        """A fresh device problem with the state (U_new, U_old, U_old); photo=None: the twin without photoionisation
        but with the same source tables."""
        from fedm_amd.cases import streamer
        from fedm_amd.device import DeviceProblem
        from fedm_amd.mesh import Marking_boundaries, Mesh
        msh = Mesh(self.mesh.coords, self.mesh.cells)
        dofs, vals = streamer.dirichlet(msh.coords)
        if photo is None:
            model = dataclasses.replace(self.dm, ext_source_degree=[1, 1])
        else:
            ph = self.photo if photo == "default" else photo
            model = dataclasses.replace(self.dm, photoionization=dataclasses.replace(ph, **change))
        prob = DeviceProblem(msh.coords, msh.cells, model, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                             dirichlet_dofs=dofs, dirichlet_vals=vals)
        prob.set_state(self.U_new, self.U_old, self.U_old)
        prob.set_step(5e-12, 4e-12)
        self._open.append(prob)
        return prob

    def close(self):
        for p in self._open:
            p.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(key):
        if key not in made:
            made[key] = Case(*key)
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def updated(cases):
    """{case key: (problem with hierarchies, problem with Jacobi alone)} after one photo_update each."""
    made = {}

    def get(key):
        if key not in made:
            case = cases(key)
            mg, jac = case.problem(), case.problem(multigrid=False)
            assert all(len(levels) >= 2 for levels in mg.photo_levels)        # real hierarchies at these sizes
            assert all(len(levels) == 1 for levels in jac.photo_levels)
            made[key] = (mg, mg.photo_update(), jac, jac.photo_update())
        return made[key]
    return get


def test_the_delaunay_mesh_is_renumbered(cases, updated):
    prob = updated(("delaunay", "closed", True))[0]
    assert (prob._order != np.arange(prob.nv)).sum() > prob.nv // 2
    sz = prob.sizes()
    assert sz["n_slices"] >= 4 and sz["assembly_variant"] in ("lds-patches/unrolled", "lds-patches", "global colouring")


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_load_vector(cases, updated, key):
    ref = cases(key).ref
    scale = np.abs(ref["g"]).max()
    assert scale > 0.0
    for prob in (updated(key)[0], updated(key)[2]):
        _, g = prob.get_photo()
        err = np.abs(g - ref["g"]).max() / scale
        print(key, "load vector", err)
        assert err < 1e-11
        assert ref["mask"].sum() > 0 and (g[ref["mask"]] == 0.0).all()


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_solves(cases, updated, key):
    ref = cases(key).ref
    free = ~ref["mask"]
    b = ref["g"]
    mg, its_mg, jac, its_jac = updated(key)
    print(key, "CG iterations with hierarchies", its_mg, "with Jacobi", its_jac)
    for prob, its in ((mg, its_mg), (jac, its_jac)):
        y, g = prob.get_photo()
        for m, A in enumerate(ref["A"]):
            rho = np.linalg.norm(b - A @ y[m]) / np.linalg.norm(b)
            lam = np.linalg.eigvalsh(A[free][:, free].toarray())
            cond = lam[-1] / lam[0]
            err = np.linalg.norm(y[m] - ref["y"][m]) / np.linalg.norm(ref["y"][m])
            print(key, "term", m, "its", its[m], "rho", rho, "cond", cond, "error", err, "bound", 2 * cond * RTOL)
            assert lam[0] > 0.0 and its[m] > 0
            assert rho <= 2.0 * RTOL
            assert err <= 2.0 * cond * RTOL
            assert (y[m][ref["mask"]] == 0.0).all()


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_table(cases, updated, key):
    case = cases(key)
    for prob in (updated(key)[0], updated(key)[2]):
        y, _ = prob.get_photo()
        want = sum(c * ym for c, ym in zip(C_TERMS, y))[case.mesh.cells]
        assert np.abs(want).max() > 0.0
        for s in (0, 1):
            got = prob.get_ext_source(s)
            assert got.shape == (case.mesh.nc, 3)
            assert (np.abs(got - want) <= 4.0 * EPS * np.abs(want)).all()
    only_e = case.problem(targets=[1])
    only_e.photo_update()
    assert only_e.get_ext_source(1).shape == (case.mesh.nc, 3)
    with pytest.raises(RuntimeError, match="no Expression source"):
        only_e.get_ext_source(0)


def _rel_rows(A, B):
    D = abs(A - B)
    scale = np.maximum(abs(B).max(axis=1).toarray().ravel(), 1e-300)
    return (sp.diags(1.0 / scale) @ D).max()


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_assembly_uses_the_table(cases, updated, key):
    """The first test of a source table together with a Poisson row and reactions, too."""
    case = cases(key)
    prob = updated(key)[0]
    tables = [prob.get_ext_source(s) for s in (0, 1)]
    twin = case.problem(photo=None)
    for s in (0, 1):
        twin.set_ext_source(s, tables[s])
    om = case.om
    saved = list(om.ext_source)
    try:
        for s in (0, 1):
            om.set_ext_source(s, 1, tables[s])
        F_ref, J_ref = om.residual_jacobian(case.U_new, case.U_old, case.U_old, 5e-12, 4e-12)
        om.ext_source = [None, None]
        F_without = om.residual(case.U_new, case.U_old, case.U_old, 5e-12, 4e-12)
    finally:
        om.ext_source = saved
    scale = np.abs(F_ref).reshape(-1, 3).max(axis=0)
    # the table is seen: without it the species rows differ by far more than the bound below
    assert (np.abs(F_ref - F_without).reshape(-1, 3) / scale)[:, :2].max() > 1e-8
    for kind in ("patch", "colour"):
        results = []
        for p in (prob, twin):
            p.set_assembly(kind)
            F, _ = p.residual()
            p.jacobian()
            J, FJ = p.jacobian_csr(), p.residual_vector()
            err_F = (np.abs(F - F_ref).reshape(-1, 3) / scale).max()
            err_J = _rel_rows(J, J_ref)
            print(key, kind, "F", err_F, "J", err_J, p.assembly_variant())
            assert err_F < 1e-11 and (np.abs(FJ - F_ref).reshape(-1, 3) / scale).max() < 1e-11
            assert err_J < 1e-10
            results.append((F, FJ, J))
        if kind == "patch":
            # The LDS-patch kernels add with fp64 LDS atomics: TWO RUNS OF ONE PROBLEM differ in the last bits (measured
            # on the MI355X: of 702 residual entries 139 differ between the two problems, by at most 5.2e-13 relative,
            # and as many between two runs of either).  Bitwise equality is asked of the kernels that have it:
            assert prob.assembly_variant() != "global colouring"
            continue
        (F1, FJ1, J1), (F2, FJ2, J2) = results
        assert prob.assembly_variant() == "global colouring"        # "bitwise reproducible" (include/fedm_hip.h)
        assert np.array_equal(F1, F2) and np.array_equal(FJ1, FJ2)
        assert np.array_equal(J1.indptr, J2.indptr) and np.array_equal(J1.indices, J2.indices)
        assert np.array_equal(J1.data, J2.data)
    prob.set_assembly("patch")


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_lag_rule(cases, key):
    case = cases(key)
    prob = case.problem(rtol=1e-8)
    prob.photo_update()
    y0, g0 = prob.get_photo()
    prob.set_state(u_new=pr.perturbed(case.U0, 23))              # u_new alone: the source does not see it
    assert prob.photo_update() == [0, 0, 0]
    y1, g1 = prob.get_photo()
    assert np.array_equal(y0, y1) and np.array_equal(g0, g1)
    prob.shift_state()                                            # u_old <- u_new: another rate
    prob.photo_update()
    y2, g2 = prob.get_photo()
    assert not np.array_equal(g0, g2) and not np.array_equal(y0, y2)
    # newton_solve updates once per shift
    prob = case.problem(rtol=1e-8)
    prob.set_state(case.U0, case.U0, case.U0)
    prob.photo_stats(reset=True)
    prob.snapshot_state()
    prob.set_step(5e-12, 1e30)
    prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    assert prob.photo_stats()["updates"] == 1
    y_step, _ = prob.get_photo()
    prob.set_step(1e-12, 1e30)                                    # a second solve at another dt, the state as it is
    prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    assert prob.photo_stats()["updates"] == 1
    prob.restore_state()
    prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    assert prob.photo_stats()["updates"] == 2
    # a rejected step (u_new <- u_old) retried with a smaller dt: the update runs again on the same u_old, finds its
    # start converged and leaves the source as it was, bit for bit
    prob.reset_state()
    prob.set_step(2.5e-12, 1e30)
    prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    assert prob.photo_stats()["updates"] == 3 and prob.last_photo_iterations == [0, 0, 0]
    assert np.array_equal(prob.get_photo()[0], y_step)
    prob.shift_state()
    prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
    assert prob.photo_stats()["updates"] == 4 and sum(prob.last_photo_iterations) > 0


@pytest.mark.parametrize("key", CASES, ids=IDS)
@pytest.mark.parametrize("multigrid", [True, False], ids=["hierarchies", "jacobi"])
def test_reproducible_and_idempotent(cases, key, multigrid):
    case = cases(key)
    a, b = case.problem(multigrid=multigrid, rtol=1e-8), case.problem(multigrid=multigrid, rtol=1e-8)
    its_a, its_b = a.photo_update(), b.photo_update()
    assert its_a == its_b and all(i > 0 for i in its_a)
    (ya, ga), (yb, gb) = a.get_photo(), b.get_photo()
    assert np.array_equal(ga, gb) and np.array_equal(ya, yb)
    for s in (0, 1):
        assert np.array_equal(a.get_ext_source(s), b.get_ext_source(s))
    assert a.photo_update() == [0, 0, 0]
    y2, g2 = a.get_photo()
    assert np.array_equal(y2, ya) and np.array_equal(g2, ga)
    st = a.photo_stats()
    assert st["updates"] == 2 and [st[f"cg_iterations_{m}"] for m in range(3)] == its_a and st["exhausted"] == 0
    assert (st["vcycles"] > 0) == multigrid


def test_other_scalar_solves_leave_the_photoionisation_alone(cases):
    """A consistent field projection and a solve of the weighting potentials run the same conjugate gradients as the
    Helmholtz terms, each with a workspace of its own: neither moves a counter, a solution or the source the assembly
    sees.  A has the two calls between its updates, B does not.  The residual is taken under the global colouring, the
    assembly that is bitwise reproducible (test_assembly_uses_the_table)."""
    case = cases(("tensor", "closed", True))
    a, b = case.problem(), case.problem()
    assert all(len(levels) >= 2 for levels in a.photo_levels)
    its_first = a.photo_update()
    assert b.photo_update() == its_first and all(i > 0 for i in its_first)
    a.set_assembly("colour")
    assert a.assembly_variant() == "global colouring"

    def seen(p):
        y, g = p.get_photo()
        F, fnorm = p.residual()
        return y.tobytes(), g.tobytes(), F.tobytes(), fnorm
    stats, before = a.photo_stats(), seen(a)
    assert stats["vcycles"] > 0

    a.fields_setup(consistent=True)
    fv = a.fields(["E_r"], projection="consistent")
    assert fv.finite and fv.cg_iterations[0] > 0
    its_psi = a.currents_setup(boundary_tags=[1, 2], max_coarse=40)
    assert len(a.currents_levels) >= 2 and len(its_psi) == 2 and all(i > 0 for i in its_psi)

    assert a.photo_stats() == stats                      # (a) entry for entry: the V-cycles of the currents' solve are not here
    assert seen(a) == before                             # (b), (c)
    its_a, its_b = a.photo_update(), b.photo_update()    # (d)
    assert its_a == its_b
    (ya, ga), (yb, gb) = a.get_photo(), b.get_photo()
    assert ya.tobytes() == yb.tobytes() and ga.tobytes() == gb.tobytes()
    assert a.photo_stats() == b.photo_stats()
    a.set_assembly("patch")


# The step runs on every case and the state is held to the oracle's on every case.  The Newton COUNT is compared wherever
# it is well defined, which the test decides from the oracle's residual history alone: no residual within 20 % of the
# tolerance.  That leaves out one case of the eight, ("delaunay", "tabulated", plane), whose residuals after iterations 3
# and 4 are 1.11e-8 and 1.38e-8 of the first: the iteration has reached its rounding floor AT the tolerance 1e-8, which
# side of it a residual falls on is noise, and the oracle stops on the step norm there (the device stops one iteration
# earlier, at the same state to 1e-15).  Should the guard ever leave out another case, the test fails.


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_a_time_step(key):
    from oracle.newton import newton_solve
    case = Case(*key, efficiency=1.0)          # see the module docstring: what the comparison needs to see the table
    try:
        om, U0 = case.om, case.U0
        ref = pr.reference(om, U0, [0], 1.0, C_TERMS, case.kappa, ZERO_TAGS)
        U_plain = U0.copy()
        its_plain, _ = newton_solve(om, U_plain, U0, U0, 5e-12, 1e30, 1e-8, 20)
        saved = list(om.ext_source)
        try:
            for s in (0, 1):
                om.set_ext_source(s, 1, ref["table"])
            U_cpu, report = U0.copy(), {}
            its_cpu, _ = newton_solve(om, U_cpu, U0, U0, 5e-12, 1e30, 1e-8, 20, report=report)
        finally:
            om.ext_source = saved
        seen = np.abs(U_cpu - U_plain).max(axis=0) / np.abs(U_cpu).max(axis=0)
        print(key, "with and without the table", seen)
        assert seen[0] > 1e-6
        history = np.array(report["residual_history"]) / report["residual_history"][0]
        print(key, "oracle's residual history", history)
        count_well_defined = bool((np.abs(history[1:] / 1e-8 - 1.0) > 0.2).all())
        prob = case.problem()
        prob.set_state(U0, U0, U0)
        prob.set_step(5e-12, 1e30)
        its, _ = prob.newton_solve(rtol=1e-8, max_it=20, ksp_rtol=1e-10)
        assert prob.photo_stats()["updates"] == 1
        d = np.abs(prob.get_state() - U_cpu).max(axis=0) / np.abs(U_cpu).max(axis=0)
        print(key, "Newton iterations", its, its_cpu, "difference", d)
        assert d.max() < 1e-9
        if count_well_defined:
            assert its == its_cpu
        else:
            assert key == ("delaunay", "tabulated", False)
    finally:
        case.close()


def test_refusals_through_the_c_abi(cases):
    import ctypes as C
    from fedm_amd import _lib, photo as photo_setup
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model
    from fedm_amd.termsum import TermSum
    case = cases(("tensor", "closed", True))
    prob = case.problem()
    lib = prob.lib
    with pytest.raises(RuntimeError, match="photoionisation set up"):
        prob.segregated_solve()
    with pytest.raises(RuntimeError, match="photoionisation set up"):
        prob.poisson_update()
    with pytest.raises(RuntimeError, match="photoionisation set up"):
        prob.newton_solve_species()

    # a level-1 hierarchy per term, as install() packs it, so that only the descriptor is at fault below
    twin = case.problem(photo=None)
    K, M = photo_setup.helmholtz_matrices(twin._coords_dev, twin._cells_dev, True, 2)
    fixed = photo_setup.zero_vertices(twin._cells_dev, twin._tags, ZERO_TAGS, twin.nv)
    from fedm_amd import amg
    keep = []
    terms = (_lib.PhotoHierarchy * 4)()
    for m in range(4):
        A = photo_setup.eliminate(K + 1e6 * M, fixed)
        n, Ac, Pc, Rc, _, held = amg._pack([(A, None)], dense_coarse=False)
        keep.append((Ac, Pc, Rc, held))
        terms[m].n_levels, terms[m].nu, terms[m].omega, terms[m].A, terms[m].P, terms[m].R = 1, 1, 0.67, Ac, Pc, Rc

    def desc(**change):
        ph = dataclasses.replace(case.photo, **{k: v for k, v in change.items() if k not in ("n_terms", "n_src")})
        d = ph.to_c()
        for k in ("n_terms", "n_src"):
            if k in change:
                setattr(d, k, change[k])
        return d

    def refused(handle, d, match):
        rc = lib.fedm_photo_setup(handle, C.byref(d), terms)
        assert rc == -2 and match in _lib.last_error(), (rc, _lib.last_error())
    assert lib.fedm_photo_setup(twin._h, C.byref(desc()), terms) == 0          # the descriptor itself is fine
    refused(twin._h, desc(n_terms=0), "0 Helmholtz terms")
    refused(twin._h, desc(n_terms=5), "5 Helmholtz terms")
    refused(twin._h, desc(kappa=[1.0, 0.0, 2.0]), "kappa[1] must be positive")
    refused(twin._h, desc(kappa=[-1.0, 1.0, 2.0]), "kappa[0] must be positive")
    refused(twin._h, desc(reactions=[1]), "source reaction index 1 out of range")
    refused(twin._h, desc(reactions=[-1]), "source reaction index -1 out of range")
    refused(twin._h, desc(n_src=0), "0 source reactions")
    refused(twin._h, desc(n_src=9), "9 source reactions")
    # the refusals left the installed set-up alone
    its = (C.c_int * 4)()
    assert lib.fedm_photo_update(twin._h, 1e-8, 500, its) == 0 and its[0] > 0

    # a target without a degree-1 source table
    no_table = DeviceProblem(case.mesh.coords, case.mesh.cells, dataclasses.replace(case.dm, ext_source_degree=[0, 1]))
    case._open.append(no_table)
    refused(no_table._h, desc(), "target species 0 has no degree-1 source table")
    deg2 = DeviceProblem(case.mesh.coords, case.mesh.cells, dataclasses.replace(case.dm, ext_source_degree=[2, 2]))
    case._open.append(deg2)
    refused(deg2._h, desc(), "target species 0 has no degree-1 source table")
    # a target with an Expression program
    from fedm_amd import forms
    ops, consts, names = forms.expression_program(forms.Expression("x[0]+x[1]", degree=1))
    twin2 = case.problem(photo=None)
    twin2.set_ext_source_program(1, ops, consts, len(names))
    refused(twin2._h, desc(), "target species 1 has an Expression program")
    assert lib.fedm_photo_setup(twin2._h, C.byref(desc(targets=[0])), terms) == 0
    with pytest.raises(RuntimeError, match="receives the photoionisation source"):
        twin2.set_ext_source_program(0, ops, consts, len(names))
    # update, get and stats without a set-up
    assert lib.fedm_photo_update(no_table._h, 1e-8, 10, its) == -2 and "fedm_photo_setup has not been called" in _lib.last_error()
    assert lib.fedm_photo_get(no_table._h, None, None) == -2
    assert lib.fedm_photo_stats(no_table._h, (C.c_int64 * 8)(), 0) == -2

    # the LMEA family
    from fedm_amd.cases import glow_discharge as gdc
    gd = gdc.Case(device_pipeline=False, T_final=1.0, nx=3, ny=3).prob
    case._open.append(gd)
    refused(gd._h, desc(), "the LMEA family has no photoionisation source")

    # ghost vertices
    ghosted = DeviceProblem(case.mesh.coords, case.mesh.cells, dataclasses.replace(case.dm, ext_source_degree=[1, 1]),
                            reorder=False, n_owned=case.mesh.nv - 5)
    case._open.append(ghosted)
    refused(ghosted._h, desc(), "one GPU")


# ---- the other instantiations of the load-vector kernel: one species without a Poisson row, three with one ------------
def _other_models(name, mesh):
    """(oracle model, device Model, state, source reactions, targets) of a model that is not the two-species streamer."""
    from oracle import streamer as ost
    from oracle.forms import LFAModel
    from oracle.mesh import mark_boundaries
    from fedm_amd.cases import streamer
    from fedm_amd.device import Model, Reaction
    from fedm_amd.termsum import TermSum
    tags = mark_boundaries(mesh, ost.BOUNDARIES)
    r, z = mesh.coords[:, 0], mesh.coords[:, 1]
    rng = np.random.default_rng(31)
    bump = np.exp(-(r ** 2 + (z - 0.008) ** 2) / (2e-3) ** 2)
    if name == "one species, no Poisson row":
        # (|E| is 1 by the element routines' convention: the rate coefficient is evaluated there)
        k = [(3.0e7, 0.5, -2.0, 1.0)]
        om = LFAModel(mesh, n_species=1, poisson=False, eq_type=["diffusion-reaction"], Z=[0.0], D=[0.1],
                      reactions=[(ost.TermSum(k), [1], [1])], facet_tags=tags, bc_type=[["zero flux"]] * 4, qdeg=2)
        dm = Model(n_species=1, poisson=False, eq_type=["diffusion-reaction"], Z=[0.0], D=[TermSum.const(0.1)],
                   reactions=[Reaction(TermSum(k), power=[1], net=[1])], bc_kind=[["zero flux"]] * 4, quadrature_degree=2)
        U = (np.log(1e13 + 1e17 * bump) + rng.normal(0, 0.2, mesh.nv))[:, None]
        return om, dm, U, [0], [0]
    base, sm = ost.build(mesh), streamer.model()
    bc = [row + ["zero flux"] for row in ost.BC_TYPE]
    om = LFAModel(mesh, n_species=3, poisson=True, eq_type=["reaction", "drift-diffusion-reaction", "reaction"],
                  Z=[1.0, -1.0, 0.0], mu=[0.0, ost.MU_E, 0.0], D=[0.0, ost.D_E, 0.0],
                  reactions=[(ost.K_ION, [0, 1, 0], [1, 1, 0]), (2.5e-19, [0, 1, 2], [0, 0, -1])],
                  facet_tags=tags, bc_type=bc, qdeg=2)
    dm = Model(n_species=3, poisson=True, eq_type=["reaction", "drift-diffusion-reaction", "reaction"], Z=[1.0, -1.0, 0.0],
               mu=[TermSum.const(0.0), sm.mu[1], TermSum.const(0.0)], D=[TermSum.const(0.0), sm.D[1], TermSum.const(0.0)],
               reactions=[Reaction(sm.reactions[0].k, power=[0, 1, 0], net=[1, 1, 0]),
                          Reaction(TermSum.const(2.5e-19), power=[0, 1, 2], net=[0, 0, -1])],
               bc_kind=bc, quadrature_degree=2)
    U2 = pr.perturbed(ost.initial_state(base), 21)
    U = np.column_stack([U2[:, 0], U2[:, 1], np.log(1e12 + 1e15 * bump) + rng.normal(0, 0.2, mesh.nv), U2[:, 2]])
    return om, dm, U, [0, 1], [0, 1, 2]


@pytest.mark.parametrize("name", ["one species, no Poisson row", "three species"])
@pytest.mark.parametrize("mesh_name", ["tensor", "delaunay"])
def test_other_species_counts(name, mesh_name):
    """photo_cell_load_kernel<1, no Poisson> and <3, Poisson> (two source reactions, one of them with a squared
    density), with their solves and tables, against the restatement; bounds as above."""
    from fedm_amd.device import DeviceProblem, Photoionization
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Marking_boundaries, Mesh
    mesh = _mesh(mesh_name)
    om, dm, U, src, targets = _other_models(name, mesh)
    h = pr.mean_edge_length(mesh.coords, mesh.cells)
    kappa = [0.1 / h, 1.0 / h, 10.0 / h]
    ref = pr.reference(om, U, src, EFFICIENCY, C_TERMS, kappa, ZERO_TAGS)
    dm.photoionization = Photoionization(reactions=src, efficiency=EFFICIENCY, c=list(C_TERMS), kappa=kappa,
                                         targets=targets, zero_tags=list(ZERO_TAGS), rtol=RTOL, max_it=2000, max_coarse=40)
    msh = Mesh(mesh.coords, mesh.cells)
    prob = DeviceProblem(msh.coords, msh.cells, dm, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES))
    try:
        prob.set_state(U + 0.01, U, U)
        its = prob.photo_update()
        y, g = prob.get_photo()
        scale = np.abs(ref["g"]).max()
        assert scale > 0.0
        err = np.abs(g - ref["g"]).max() / scale
        print(name, mesh_name, "load vector", err, "CG iterations", its)
        assert err < 1e-11 and (g[ref["mask"]] == 0.0).all()
        free = ~ref["mask"]
        for m, A in enumerate(ref["A"]):
            rho = np.linalg.norm(ref["g"] - A @ y[m]) / np.linalg.norm(ref["g"])
            lam = np.linalg.eigvalsh(A[free][:, free].toarray())
            e = np.linalg.norm(y[m] - ref["y"][m]) / np.linalg.norm(ref["y"][m])
            print(name, mesh_name, "term", m, "rho", rho, "error", e, "bound", 2 * lam[-1] / lam[0] * RTOL)
            assert rho <= 2.0 * RTOL and e <= 2.0 * lam[-1] / lam[0] * RTOL
        want = sum(c * ym for c, ym in zip(C_TERMS, y))[mesh.cells]
        for s in targets:
            assert (np.abs(prob.get_ext_source(s) - want) <= 4.0 * EPS * np.abs(want)).all()
        # the assembly with these tables against the oracle carrying the same ones
        for s in targets:
            om.set_ext_source(s, 1, prob.get_ext_source(s))
        F_ref, J_ref = om.residual_jacobian(U + 0.01, U, U, 5e-12, 4e-12)
        prob.set_step(5e-12, 4e-12)
        F, _ = prob.residual()
        prob.jacobian()
        fscale = np.abs(F_ref).reshape(-1, om.neq).max(axis=0)
        assert (np.abs(F - F_ref).reshape(-1, om.neq) / fscale).max() < 1e-11
        assert _rel_rows(prob.jacobian_csr(), J_ref) < 1e-10
    finally:
        prob.close()


def test_an_update_that_meets_a_nan_leaves_a_clean_start(cases):
    """A state that is not finite gives FEDM_DIVERGED_NAN; the terms go back to 0, the tables are finite, and the next
    update on a sound state converges as a first one does."""
    case = cases(("tensor", "closed", True))
    prob = case.problem(rtol=1e-8)
    first = prob.photo_update()
    y_first, _ = prob.get_photo()
    bad = case.U_old.copy()
    bad[7, 1] = np.nan
    prob.set_state(u_old=bad)
    with pytest.raises(RuntimeError, match="NaN or Inf"):
        prob.photo_update()
    y, _ = prob.get_photo()
    assert (y == 0.0).all()
    for s in (0, 1):
        assert (prob.get_ext_source(s) == 0.0).all()
    prob.set_state(u_old=case.U_old)
    again = prob.photo_update()
    y_again, _ = prob.get_photo()
    assert again == first and np.array_equal(y_again, y_first)
