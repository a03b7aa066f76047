"""Tabulated E/N coefficients looked up in the LFA element routines, against the oracle.

The oracle takes the tables through tests/tabulated_reference.py (a subclass of its own TermSum); the device through
TermSum.table and fedm_ctx_create_tabulated.  Model: the streamer with mu_e and D_e tabulated and
k = T_alpha * T_mu * E (two table factors), 9 log-spaced knots between the 10 % and 90 % quantiles of the cells' |E|
of the perturbed state -- both clamped regions and all segments hold cells.  Tolerances are those the closed-form
model is held to (tests/test_gpu_parity.py): the look-up adds rounding only.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import tabulated_reference as tr

pytestmark = pytest.mark.gpu

PATHS = {"lds-patches": {"FEDM_ASSEMBLY_LEAN": "2"}, "lds-patches/unrolled": {"FEDM_ASSEMBLY_LEAN": "0"},
         "global colouring": {"FEDM_ASSEMBLY": "colour"}}
STEPS = [(5e-12, 1e30), (5e-12, 4e-12)]


def _perturbed(U0, seed):
    rng = np.random.default_rng(seed)
    U = U0.copy()
    U[:, 0] += rng.normal(0, 0.05, U.shape[0])
    U[:, 1] += rng.normal(0, 0.3, U.shape[0])
    U[:, 2] += rng.normal(0, 20.0, U.shape[0])
    return U


def _rel_rows(A, B):
    D = abs(A - B)
    scale = np.maximum(abs(B).max(axis=1).toarray().ravel(), 1e-300)
    return (sp.diags(1.0 / scale) @ D).max()


@pytest.fixture(scope="module")
def tensor_case():
    """The 20 x 20 graded mesh of test_gpu_parity.py's streamer_setup, its perturbed states, the knots and the oracle's
    F and J for both step pairs (computed once, never changed)."""
    from oracle import streamer as ost
    from oracle.mesh import graded_axis, rectangle_right
    n = 20
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, n, n, xs=graded_axis(ost.BOX, n, 6.0))
    closed = ost.build(mesh)
    U0 = ost.initial_state(closed)
    U, Uo, Uo1 = _perturbed(U0, 1), _perturbed(U0, 2), _perturbed(U0, 3)
    Em = closed.cell_fields(U)[2]
    x = tr.quantile_knots(Em)
    om = tr.oracle_streamer(mesh, x)
    tr.assert_knots_exercise_the_lookup(x, om.cell_fields(U)[2])
    ref = {st: om.residual_jacobian(U, Uo, Uo1, *st) for st in STEPS}
    return dict(mesh=mesh, om=om, U0=U0, states=(U, Uo, Uo1), x=x, ref=ref)


def _against_the_oracle(prob, states, dt, dt_old, F_cpu, J_cpu, path):
    U, Uo, Uo1 = states
    prob.set_state(U, Uo, Uo1)
    prob.set_step(dt, dt_old)
    F_gpu, fnorm = prob.residual()
    eF = np.abs(F_gpu - F_cpu).max() / np.abs(F_cpu).max()
    prob.jacobian()
    launched = prob.launched_assembly()
    eJ = _rel_rows(prob.jacobian_csr(), J_cpu)
    xv = np.random.default_rng(5).normal(size=prob.n)
    y, yc = prob.spmv(xv), J_cpu @ xv
    eP = np.abs(y - yc).max() / np.abs(yc).max()
    print(f"[tabulated] {path} dt_old {dt_old:g}: F {eF:.2e} J {eJ:.2e} product {eP:.2e} launched {launched}", flush=True)
    for what in ("residual", "jacobian"):
        assert launched[what]["variant"] == path     # in particular never the one-pass kernel
    assert prob.assembly_variant() == path
    assert eF < 1e-11
    assert fnorm == pytest.approx(np.linalg.norm(F_cpu), rel=1e-11)
    assert eJ < 1e-10
    assert eP < 1e-11


@pytest.mark.parametrize("path", list(PATHS))
def test_residual_jacobian_and_product_against_the_oracle(tensor_case, monkeypatch, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    c = tensor_case
    prob = tr.device_streamer_problem(c["mesh"].coords, c["mesh"].cells, tr.device_streamer_model(c["x"]))
    for st in STEPS:
        _against_the_oracle(prob, c["states"], *st, *c["ref"][st], path)
    prob.close()


@pytest.fixture(scope="module")
def unstructured_case():
    """The locally refined mesh of test_row_at_a_time_assembly...: turned cells, patches of 256 threads; its state,
    knots from its own |E|, and the oracle's F and J for both step pairs (computed once, never changed)."""
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.cases import streamer
    msh = streamer.refined_mesh(60e-6)
    omesh = OMesh(msh.coords, msh.cells)
    nv = msh.coords.shape[0]
    rng = np.random.default_rng(3)
    xs, ys = msh.coords[:, 0] / streamer.BOX, msh.coords[:, 1] / streamer.BOX
    U = np.zeros((nv, 3))
    U[:, 0] = 30.0 + 2.0 * np.sin(5 * xs) * np.cos(3 * ys)
    U[:, 1] = 28.0 + 3.0 * np.cos(4 * xs) * np.sin(6 * ys)
    U[:, 2] = streamer.U_W * ys + 50.0 * np.sin(3 * xs) * np.sin(np.pi * ys)
    Uo, Uo1 = U + 0.01 * rng.standard_normal(U.shape), U + 0.02 * rng.standard_normal(U.shape)
    Em = ost.build(omesh).cell_fields(U)[2]
    x = tr.quantile_knots(Em)
    tr.assert_knots_exercise_the_lookup(x, Em)
    om = tr.oracle_streamer(omesh, x)
    ref = {st: om.residual_jacobian(U, Uo, Uo1, *st) for st in STEPS}
    return dict(mesh=msh, states=(U, Uo, Uo1), x=x, ref=ref)


@pytest.mark.parametrize("path", list(PATHS))
def test_unstructured_mesh_against_the_oracle(unstructured_case, monkeypatch, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    c = unstructured_case
    prob = tr.device_streamer_problem(c["mesh"].coords, c["mesh"].cells, tr.device_streamer_model(c["x"]))
    for st in STEPS:
        _against_the_oracle(prob, c["states"], *st, *c["ref"][st], path)
    prob.close()


def test_a_straight_line_as_a_table_is_the_term_sum(tensor_case):
    """y = a + b x on two knots outside the field range equals the term sum a + b E: device against device."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import Model, Reaction
    from fedm_amd.termsum import TermSum, parse
    c = tensor_case
    U, Uo, Uo1 = c["states"]
    knots = np.array([1.0e4, 1.0e8])
    Em = c["om"].cell_fields(U)[2]
    assert knots[0] < Em.min() and Em.max() < knots[1]
    a, b, d0, d1 = 0.05, -2.0e-9, 0.1, 3.0e-8
    out = {}
    for kind in ("table", "termsum"):
        if kind == "table":
            mu, D = TermSum.table(knots, a + b * knots), TermSum.table(knots, d0 + d1 * knots)
        else:
            mu, D = parse(f"{a!r} + {b!r}*E_m"), parse(f"{d0!r} + {d1!r}*E_m")
        model = Model(n_species=2, poisson=True, eq_type=["reaction", "drift-diffusion-reaction"], Z=[1.0, -1.0],
                      mu=[TermSum.const(0.0), mu], D=[TermSum.const(0.0), D],
                      reactions=[Reaction(parse(streamer.ALPHA) * mu * TermSum.field(), power=[0, 1], net=[1, 1])],
                      bc_kind=streamer.BC_TYPE, quadrature_degree=2)
        prob = tr.device_streamer_problem(c["mesh"].coords, c["mesh"].cells, model)
        prob.set_state(U, Uo, Uo1)
        prob.set_step(5e-12, 4e-12)
        prob.jacobian()
        out[kind] = (prob.residual_vector(), prob.jacobian_csr(), prob.assembly_variant())
        prob.close()
    (F1, J1, v1), (F0, J0, v0) = out["table"], out["termsum"]
    eF, eJ = np.abs(F1 - F0).max() / np.abs(F0).max(), _rel_rows(J1, J0)
    print(f"[tabulated] line as table: F {eF:.2e} J {eJ:.2e} ({v1} against {v0})", flush=True)
    assert v1 == "lds-patches"
    # the slope (y1 - y0) / (x1 - x0) and the product a + slope (E - x0) round differently from a + b E: a few ulp of
    # the coefficient, far below the 1e-11 / 1e-10 two implementations of the same tensors are held to
    assert eF < 1e-11 and eJ < 1e-10


def test_newton_step_against_the_oracle(tensor_case):
    """Jacobi-GMRES, then field split + multigrid: same iteration count as oracle.newton and 1e-8, as
    test_four_species_and_poisson_against_the_oracle."""
    from oracle.newton import newton_solve
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    c = tensor_case
    U0 = c["U0"]
    tr.assert_knots_exercise_the_lookup(c["x"], c["om"].cell_fields(U0)[2])
    U_cpu = U0.copy()
    its_cpu, _ = newton_solve(c["om"], U_cpu, U0, U0, 5e-12, 1e30, 1e-8, 25)
    prob = tr.device_streamer_problem(c["mesh"].coords, c["mesh"].cells, tr.device_streamer_model(c["x"]))
    for split in (False, True):
        prob.set_state(U0, U0, U0)
        prob.set_step(5e-12, 1e30)
        if split:
            prob.setup_multigrid(**streamer.MULTIGRID)
            prob.set_fieldsplit(chebyshev_weights(6))
        its, _ = prob.newton_solve(rtol=1e-8, max_it=25, ksp_rtol=1e-10, ksp_max_it=2000)
        d = np.abs(prob.get_state() - U_cpu).max(axis=0) / np.abs(U_cpu).max(axis=0)
        print(f"[tabulated] newton split={split}: its {its} (oracle {its_cpu}) diff {d}", flush=True)
        assert its == its_cpu, (split, its, its_cpu)
        assert d.max() < 1e-8, (split, d)
    assert prob.launched_assembly()["jacobian"]["variant"] == "lds-patches"
    prob.close()


@pytest.mark.parametrize("lean", ["2", "0"])
def test_four_species_with_four_tables_and_a_one_knot_table(monkeypatch, lean):
    """tests/lfa_models.py's four-species model with the electrons' mu and D, the ions' D and the metastables' D
    tabulated (table indices 0..3; the metastables' table has ONE knot: a constant) and a two-factor ionisation rate."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem
    from fedm_amd.mesh import Marking_boundaries
    from fedm_amd.termsum import TermSum
    from lfa_models import four_species_problem
    monkeypatch.setenv("FEDM_ASSEMBLY_LEAN", lean)
    m, closed_prob, om, ddofs, dvals = four_species_problem()
    model = closed_prob.model
    closed_prob.close()
    nv = m.coords.shape[0]
    rng = np.random.default_rng(4)
    xs, ys = m.coords[:, 0] / streamer.BOX, m.coords[:, 1] / streamer.BOX
    U = np.zeros((nv, 5))
    U[:, 0] = 27.0 + np.sin(4 * xs) * np.cos(2 * ys)
    U[:, 1] = 30.0 + 2.0 * np.sin(5 * xs) * np.cos(3 * ys)
    U[:, 2] = 25.0 + np.sin(3 * xs + 2 * ys)
    U[:, 3] = 29.0 + 2.0 * np.cos(4 * xs) * np.sin(6 * ys)
    U[:, 4] = streamer.U_W * ys + 50.0 * np.sin(3 * xs) * np.sin(np.pi * ys)
    U.ravel()[ddofs] = dvals
    Uo, Uo1 = U + 0.01 * rng.standard_normal(U.shape), U + 0.02 * rng.standard_normal(U.shape)
    Em = om.cell_fields(U)[2]
    x = tr.quantile_knots(Em)
    tr.assert_knots_exercise_the_lookup(x, Em)
    mu_y, D_y, alpha_y = tr.closed_forms(x)
    x_ion = np.sqrt(x[:-1:2] * x[1::2])                      # another grid: a table of its own
    tr.assert_knots_exercise_the_lookup(x_ion, Em)
    ion_y = 3e-6 * (1.0 + 0.2 * np.log(x_ion / x_ion[0]))
    one = [(1.0, 0.0, 0.0, 0.0)]
    om.D[0] = tr.TabulatedTermSum(one, [([x[3]], [5e-4])])
    om.D[1] = tr.TabulatedTermSum(one, [(x_ion, ion_y)])
    om.mu[3] = tr.TabulatedTermSum(one, [(x, mu_y)])
    om.D[3] = tr.TabulatedTermSum(one, [(x, D_y)])
    k = tr.TabulatedTermSum([(1.0, 1.0, 0.0, 0.0)], [(x, alpha_y), (x, mu_y)])
    om.reactions[0] = (k, om.reactions[0][1], om.reactions[0][2])
    mu_e = TermSum.table(x, mu_y)
    model.mu = list(model.mu[:3]) + [mu_e]
    model.D = [TermSum.table([x[3]], [5e-4]), TermSum.table(x_ion, ion_y), model.D[2], TermSum.table(x, D_y)]
    model.reactions[0].k = TermSum.table(x, alpha_y) * mu_e * TermSum.field()
    md, ptr, _, _ = model.to_c_tabulated()
    assert ptr.size - 1 == 5 and md.D[0].pad_ > 0 and md.k[0].pad_ >> 16 > 0        # five distinct tables
    prob = DeviceProblem(m.coords, m.cells, model, facet_tags=Marking_boundaries(m, streamer.BOUNDARIES),
                         dirichlet_dofs=ddofs.astype(np.int32), dirichlet_vals=dvals)
    dt, dt_old = 5e-12, 4e-12
    prob.set_state(U, Uo, Uo1)
    prob.set_step(dt, dt_old)
    F_gpu, fnorm = prob.residual()
    F_cpu, J_cpu = om.residual_jacobian(U, Uo, Uo1, dt, dt_old)
    scale = np.abs(F_cpu).reshape(-1, 5).max(axis=0)
    eF = (np.abs(F_gpu - F_cpu).reshape(-1, 5) / scale).max()
    prob.jacobian()
    eJ = _rel_rows(prob.jacobian_csr(), J_cpu)
    print(f"[tabulated] four species lean {lean}: F {eF:.2e} J {eJ:.2e}", flush=True)
    assert prob.launched_assembly()["jacobian"]["variant"] == ("lds-patches" if lean == "2" else "lds-patches/unrolled")
    assert eF < 1e-11 and eJ < 1e-10
    prob.close()


def test_species_only_assembly_and_a_segregated_step(tensor_case):
    """The species planes of fedm_debug_species_assembly equal the coupled assembly's (a table model takes the full
    second-generation assembly there), and segregated_solve runs."""
    import segregated_reference as sr
    c = tensor_case
    U, Uo, Uo1 = c["states"]
    prob = tr.device_streamer_problem(c["mesh"].coords, c["mesh"].cells, tr.device_streamer_model(c["x"]))
    prob.set_state(U, Uo, Uo1)
    prob.set_step(5e-12, 4e-12)
    prob.jacobian()
    F, J = prob.residual_vector(), prob.jacobian_csr()
    assert prob.species_assembly(jacobian=True) is False          # the full assembly, not the one-pass kernel
    Fs, Js = prob.residual_vector(), prob.jacobian_csr()
    iu, ip = sr.block_indices(U.size, 3)
    # the same kernels twice: equal up to the order of the LDS atomics' sums (the bounds two implementations of the
    # same tensors are held to in test_row_at_a_time_assembly_matches_the_unrolled_element)
    assert np.all(Fs[ip] == 0.0)
    assert np.abs(Fs[iu] - F[iu]).max() <= 1e-12 * np.abs(F[iu]).max()
    Juu, Juu_s = sr.species_block(J, 3), sr.species_block(Js, 3)
    rowmax = abs(Juu).max(axis=1).toarray().ravel()
    assert (abs(Juu_s - Juu).max(axis=1).toarray().ravel() <= 1e-11 * rowmax + 1e-300).all()
    assert prob.launched_assembly()["jacobian"]["variant"] == "lds-patches"
    U0 = c["U0"]
    prob.set_state(U0, U0, U0)
    prob.set_step(5e-12, 1e30)
    its, _ = prob.segregated_solve(rtol=1e-8, max_it=25, ksp_rtol=1e-10)
    new = prob.get_state()
    assert 0 < its <= 25 and np.isfinite(new).all() and np.abs(new - U0).max() > 0.0
    # against the oracle's species rows at the state reached: the species Newton converged on the tabulated model
    F_cpu = c["om"].residual(new.reshape(U0.shape), U0, U0, 5e-12, 1e30)
    F0 = c["om"].residual(U0, U0, U0, 5e-12, 1e30)
    assert np.linalg.norm(F_cpu[iu]) <= 1e-6 * np.linalg.norm(F0[iu])
    prob.close()


def _raw_create(model, mesh, n_tables, ptr, x, y, tabulated=True):
    """fedm_ctx_create[_tabulated] through the ABI with the arrays as given (None: NULL)."""
    from fedm_amd import _lib
    from fedm_amd.cases import streamer
    lib = _lib.load()
    md = model if isinstance(model, _lib.ModelDesc) else model.to_c()
    coords = np.ascontiguousarray(mesh.coords, dtype=np.float64)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int32)
    dofs, vals = streamer.dirichlet(coords)
    mdesc = _lib.MeshDesc()
    mdesc.n_vertices, mdesc.n_cells = coords.shape[0], cells.shape[0]
    mdesc.coords = coords.ctypes.data_as(C.POINTER(C.c_double))
    mdesc.cells = cells.ctypes.data_as(C.POINTER(C.c_int32))
    mdesc.n_dirichlet = dofs.size
    mdesc.dirichlet_dofs = dofs.ctypes.data_as(C.POINTER(C.c_int32))
    mdesc.dirichlet_vals = vals.ctypes.data_as(C.POINTER(C.c_double))
    handle = C.c_void_p()
    keep = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((ptr, np.int32), (x, float), (y, float))]
    p = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double)) for a in keep]
    if tabulated:
        rc = lib.fedm_ctx_create_tabulated(C.byref(mdesc), C.byref(md), n_tables, p[0], p[1], p[2], 0, C.byref(handle))
    else:
        rc = lib.fedm_ctx_create(C.byref(mdesc), C.byref(md), 0, C.byref(handle))
    msg = _lib.last_error()
    if rc == 0:
        lib.fedm_ctx_destroy(handle)
    return rc, msg, handle.value


def test_refusals_through_the_abi(tensor_case):
    """Every refusal of fedm_ctx_create_tabulated: a negative return, a message that names the trouble, no context."""
    from fedm_amd.device import Model
    from fedm_amd.termsum import TermSum
    c = tensor_case
    mesh, x = c["mesh"], c["x"]
    model = tr.device_streamer_model(x)
    md, ptr, tx, ty = model.to_c_tabulated()
    n = ptr.size - 1
    assert n == 3
    rc, msg, h = _raw_create(md, mesh, n, ptr, tx, ty)
    assert rc == 0, msg                                               # the arrays as they are: accepted
    nan_y, inf_x, flat_x = ty.copy(), tx.copy(), tx.copy()
    nan_y[2] = np.nan
    inf_x[ptr[3] - 1] = np.inf
    flat_x[ptr[1] + 4] = flat_x[ptr[1] + 3]
    empty = ptr.copy()
    empty[1] = 0
    no_poisson = Model(n_species=1, poisson=False, eq_type=["diffusion-reaction"], Z=[0.0],
                       D=[TermSum.table(x, np.ones_like(x))], quadrature_degree=2)
    md1, ptr1, tx1, ty1 = no_poisson.to_c_tabulated()
    cases = [("beyond n_tables", (md, n - 1, ptr[:n], tx, ty), "refers to table 2"),
             ("empty table", (md, n, empty, tx, ty), "table 0 has no entries"),
             ("knots not increasing", (md, n, ptr, flat_x, ty), "knots of table 1 do not strictly increase"),
             ("NaN value", (md, n, ptr, tx, nan_y), "table 0 has a knot or value that is not finite"),
             ("infinite knot", (md, n, ptr, inf_x, ty), "table 2 has a knot or value that is not finite"),
             ("tab_ptr not from 0", (md, n, ptr + 1, tx, ty), "tab_ptr must start at 0"),
             ("tab_ptr decreasing", (md, n, np.array([0, 9, 5, 27]), tx, ty), "tab_ptr must not decrease"),
             ("null tab_ptr", (md, n, None, tx, ty), "null tab_ptr"),
             ("null arrays", (md, n, ptr, None, ty), "null table arrays"),
             ("too many tables", (md, 17, np.arange(18), tx, ty), "at most 16"),
             ("no Poisson equation", (md1, 1, ptr1, tx1, ty1), "no Poisson equation")]
    for name, args, expect in cases:
        rc, msg, h = _raw_create(*args[:1], mesh, *args[1:])
        print(f"[tabulated] refusal {name}: {rc} {msg!r}", flush=True)
        assert rc < 0 and h is None and expect in msg and "fedm_ctx_create_tabulated" in msg, name
    rc, msg, h = _raw_create(md, mesh, 0, None, None, None, tabulated=False)
    print(f"[tabulated] refusal plain creator: {rc} {msg!r}", flush=True)
    assert rc < 0 and h is None and "refers to table" in msg and msg.startswith("fedm_ctx_create:")


def test_example_script_with_the_tabulated_deck(tmp_path):
    """examples/streamer_discharge.py --model tabulated_model, four steps on the 24 x 24 graded mesh: the same error
    log and state as the case module on the same deck, and as the oracle's time loop (oracle/streamer.py: run) whose
    Newton solves take the same tables -- at the tolerances of test_example_script_in_fedm_shape (log rows 1e-6,
    state 1e-8)."""
    import importlib.util
    from pathlib import Path
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from oracle.newton import newton_solve
    from fedm_amd.cases import streamer
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("ex_streamer_tab", root / "examples" / "streamer_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    state, log = mod.main(cells=24, end_time=2e-11, output_dir=tmp_path, quiet=True, model="tabulated_model")
    rows = np.loadtxt(log).reshape(-1, 3)
    msh = streamer.mesh(24, 4.0)
    prob = streamer.device_problem(msh.coords, msh.cells, deck_model="tabulated_model")
    assert prob.assembly_variant() == "lds-patches"
    ref = streamer.run(prob, T_final=2e-11)
    case_state = prob.get_state()
    launched = prob.launched_assembly()
    prob.close()
    omesh = OMesh(msh.coords, msh.cells)
    om = tr.oracle_model_of(omesh, streamer.model_from_deck(model_name="tabulated_model"))
    U_cpu, st, _, _ = ost.run(mesh=omesh, T_final=2e-11,
                              solver=lambda _m, Uw, Uo, Uo1, dt, dto: newton_solve(om, Uw, Uo, Uo1, dt, dto, 1e-4, 20))
    orows = np.array(st.log)
    d_case = np.abs(state - case_state).max(axis=0) / np.abs(case_state).max(axis=0)
    d_cpu = np.abs(state - U_cpu).max(axis=0) / np.abs(U_cpu).max(axis=0)
    print(f"[tabulated] example: rows {rows.tolist()}\n[tabulated] oracle rows {orows.tolist()}\n"
          f"[tabulated] example against case module {d_case}, against the oracle loop {d_cpu}; "
          f"rows against the oracle {np.abs(rows / orows - 1.0).max():.2e}", flush=True)
    assert launched["jacobian"]["variant"] == "lds-patches"
    assert rows.shape == (4, 3) and np.allclose(rows, np.array(ref["log"]), rtol=1e-6)
    assert np.allclose(state, case_state, rtol=1e-8, atol=1e-8)
    assert orows.shape == (4, 3) and np.allclose(rows, orows, rtol=1e-6)
    assert np.allclose(state, U_cpu, rtol=1e-8, atol=1e-8)
