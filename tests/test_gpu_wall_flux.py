"""'flux source' walls of LFA models on the device against the numpy restatement (tests/wall_flux_reference.py).

Model: ions (drift-diffusion, Z = +1, mu = 2e-4, D = 3e-6) and the deck's electrons with its ionisation, plus Poisson.
The electrodes are the walls: z = 0 (tag 1; ref 0.3, gamma 0.07) and z = BOX (tag 2; ref 0, gamma 0), 'flux source' for
both species; r = BOX (tag 4) keeps the deck's Neumann condition for the electrons, so both facet terms run in one
kernel; the axis (tag 3) is zero flux.  The state's potential makes E.n take both signs on every wall
(wall_flux_reference.wall_state, assert_preconditions).  Tolerances are those two implementations of the same tensors
are held to in tests/test_gpu_tabulated.py.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import wall_flux_reference as wr

pytestmark = pytest.mark.gpu

# every assembly path a wall model can take: test_gpu_tabulated.py's, and the default (which for every other
# two-species model of this shape is the one-pass kernel and for a wall model must not be)
PATHS = {"lds-patches": {"FEDM_ASSEMBLY_LEAN": "2"}, "lds-patches/unrolled": {"FEDM_ASSEMBLY_LEAN": "0"},
         "global colouring": {"FEDM_ASSEMBLY": "colour"}, "default": {}}
DT = (5e-12, 4e-12)


def _rel_rows(A, B):
    D = abs(A - B)
    scale = np.maximum(abs(B).max(axis=1).toarray().ravel(), 1e-300)
    return (sp.diags(1.0 / scale) @ D).max()


def _case(coords, cells, **model_kw):
    """Mesh, restatement, states and the restatement's F and J (computed once, never changed)."""
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.mesh import Mesh
    msh = Mesh(coords, cells)
    om = wr.set_dirichlet(wr.oracle_two_species(OMesh(msh.coords, msh.cells), **model_kw), msh.coords)
    log = model_kw.get("log", True)
    U = wr.wall_state(msh.coords, log=log)
    info = wr.assert_preconditions(om, U)
    rng = np.random.default_rng(3)
    if log:
        Uo, Uo1 = U - 0.01 * rng.random(U.shape), U - 0.02 * rng.random(U.shape)
    else:                     # densities: a relative change
        Uo, Uo1 = U * (1.0 - 0.01 * rng.random(U.shape)), U * (1.0 - 0.02 * rng.random(U.shape))
    F, J = om.residual_jacobian(U, Uo, Uo1, *DT)
    return dict(mesh=msh, om=om, states=(U, Uo, Uo1), F=F, J=J, info=info)


@pytest.fixture(scope="module")
def tensor_case():
    from fedm_amd.cases import streamer
    msh = streamer.mesh(20, 2.0)
    return _case(msh.coords, msh.cells)


@pytest.fixture(scope="module")
def unstructured_case():
    from fedm_amd.cases import streamer
    msh = streamer.refined_mesh(60e-6)
    return _case(msh.coords, msh.cells)


@pytest.fixture(scope="module")
def cells192_case():
    """140 tagged facets: two 128-thread facet blocks of the fused facet/Dirichlet kernel, the second partial."""
    import limit_meshes
    c = _case(*limit_meshes.build("cells192"))
    assert (c["om"].facet_tags > 0).sum() == 140
    return c


def _against_the_restatement(prob, c, what, expect_variant=None):
    U, Uo, Uo1 = c["states"]
    F_cpu, J_cpu = c["F"], c["J"]
    prob.set_state(U, Uo, Uo1)
    prob.set_step(*DT)
    F_gpu, fnorm = prob.residual()
    eF = np.abs(F_gpu - F_cpu).max() / np.abs(F_cpu).max()
    # twice in a row: a plane that the assembly keeps although the facets add to it shows on the second one
    eJ = []
    for _ in range(2):
        prob.jacobian()
        eJ.append(_rel_rows(prob.jacobian_csr(), J_cpu))
    launched = prob.launched_assembly()
    xv = np.random.default_rng(5).normal(size=prob.n)
    y, yc = prob.spmv(xv), J_cpu @ xv
    eP = np.abs(y - yc).max() / np.abs(yc).max()
    print(f"[walls] {what}: F {eF:.2e} J {eJ[0]:.2e} {eJ[1]:.2e} product {eP:.2e} launched {launched}", flush=True)
    for kind in ("residual", "jacobian"):
        assert launched[kind]["variant"] != "lds-patches/one-pass"
        if expect_variant is not None:
            assert launched[kind]["variant"] == expect_variant
    assert eF < 1e-11
    assert fnorm == pytest.approx(np.linalg.norm(F_cpu), rel=1e-11)
    assert max(eJ) < 1e-10
    assert eP < 1e-11


def _run_paths(c, monkeypatch, path, what, pin_variant=True):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    prob = wr.device_problem(c["mesh"].coords, c["mesh"].cells, wr.device_two_species_model())
    expect = ("lds-patches" if path == "default" else path) if pin_variant else None
    try:
        _against_the_restatement(prob, c, f"{what} {path}", expect)
    finally:
        prob.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_tensor_mesh_against_the_restatement(tensor_case, monkeypatch, path):
    _run_paths(tensor_case, monkeypatch, path, "tensor 20x20")


@pytest.mark.parametrize("path", list(PATHS))
def test_unstructured_mesh_against_the_restatement(unstructured_case, monkeypatch, path):
    _run_paths(unstructured_case, monkeypatch, path, "unstructured")


@pytest.mark.parametrize("path", list(PATHS))
def test_two_facet_blocks_against_the_restatement(cells192_case, monkeypatch, path):
    _run_paths(cells192_case, monkeypatch, path, "cells192 reordered", pin_variant=False)


def test_the_emission_plane_is_neither_kept_nor_skipped(tensor_case):
    """(electrons, ions) = plane (1, 0), bit 3 of fedm_plane_masks' zero mask: structurally zero without emission,
    filled by the cathode's facets with it.  The product J x equals jacobian_csr() @ x: the SpMV skips nothing that
    the assembly filled."""
    c = tensor_case
    U, Uo, Uo1 = c["states"]
    for gamma, zero_expected in ((0.07, 0), (0.0, 8)):
        prob = wr.device_problem(c["mesh"].coords, c["mesh"].cells, wr.device_two_species_model(gamma_cathode=gamma))
        kept, zero = prob.plane_masks()
        print(f"[walls] gamma {gamma}: kept {kept:#b} zero {zero:#b}", flush=True)
        assert zero & 8 == zero_expected and zero & 2 == 0       # (ions, electrons): the ionisation couples them
        assert (kept >> 3) & 1 == (1 if zero_expected and kept else 0)
        if gamma:
            prob.set_state(U, Uo, Uo1)
            prob.set_step(*DT)
            prob.jacobian()
            J = prob.jacobian_csr()
            plane = J[1::3][:, 0::3]
            assert abs(plane).max() > 0.0
            xv = np.random.default_rng(7).normal(size=prob.n)
            y, yc = prob.spmv(xv), J @ xv
            assert np.abs(y - yc).max() <= 1e-12 * np.abs(yc).max()
        prob.close()


def test_linear_representation(tensor_case):
    """log_representation=False: n = u and grad n = grad u in the wall terms, on the generic element's kernels."""
    msh = tensor_case["mesh"]
    c = _case(msh.coords, msh.cells, log=False)
    prob = wr.device_problem(msh.coords, msh.cells, wr.device_two_species_model(log=False))
    try:
        _against_the_restatement(prob, c, "linear representation")
    finally:
        prob.close()


def test_tabulated_coefficients_in_a_wall_model(tensor_case):
    """mu_e and D_e as tables (tabulated_reference.quantile_knots): the wall terms look them up through
    termsum_eval<TAB>, as the Neumann term does."""
    import tabulated_reference as tr
    from fedm_amd.termsum import TermSum
    c0 = tensor_case
    msh = c0["mesh"]
    Em = c0["om"].cell_fields(c0["states"][0])[2]
    x = tr.quantile_knots(Em)
    tr.assert_knots_exercise_the_lookup(x, Em)
    mu_y, D_y, _ = tr.closed_forms(x)
    one = [(1.0, 0.0, 0.0, 0.0)]
    c = _case(msh.coords, msh.cells, mu_e=tr.TabulatedTermSum(one, [(x, mu_y)]), D_e=tr.TabulatedTermSum(one, [(x, D_y)]))
    model = wr.device_two_species_model(mu_e=TermSum.table(x, mu_y), D_e=TermSum.table(x, D_y))
    prob = wr.device_problem(msh.coords, msh.cells, model)
    _against_the_restatement(prob, c, "tabulated mu_e, D_e", "lds-patches")
    prob.close()


def test_four_species_with_walls():
    """tests/lfa_models.py's four-species model with the same walls: the metastable is 'diffusion-reaction' (the thermal
    term alone), the negative ion has a constant drift velocity and stays at zero flux."""
    m, model, om, ddofs, dvals = wr.four_species_pair()
    U = wr.wall_state(m.coords, neq=5)
    U.ravel()[ddofs] = dvals
    wr.assert_preconditions(om, U)
    rng = np.random.default_rng(4)
    Uo, Uo1 = U - 0.01 * rng.random(U.shape), U - 0.02 * rng.random(U.shape)
    F_cpu, J_cpu = om.residual_jacobian(U, Uo, Uo1, *DT)
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem
    from fedm_amd.mesh import Marking_boundaries
    prob = DeviceProblem(m.coords, m.cells, model, facet_tags=Marking_boundaries(m, streamer.BOUNDARIES),
                         dirichlet_dofs=ddofs.astype(np.int32), dirichlet_vals=dvals)
    prob.set_state(U, Uo, Uo1)
    prob.set_step(*DT)
    F_gpu, _ = prob.residual()
    scale = np.abs(F_cpu).reshape(-1, 5).max(axis=0)
    eF = (np.abs(F_gpu - F_cpu).reshape(-1, 5) / scale).max()
    eJ = []
    for _ in range(2):
        prob.jacobian()
        eJ.append(_rel_rows(prob.jacobian_csr(), J_cpu))
    print(f"[walls] four species: F {eF:.2e} J {eJ[0]:.2e} {eJ[1]:.2e} launched {prob.launched_assembly()}", flush=True)
    prob.close()
    assert eF < 1e-11 and max(eJ) < 1e-10


def test_newton_step_against_the_restatement(tensor_case):
    """Jacobi-GMRES, then field split + multigrid: the iteration count of oracle.newton on the restatement and 1e-8,
    as test_gpu_tabulated.py's test_newton_step_against_the_oracle."""
    from oracle import streamer as ost
    from oracle.newton import newton_solve
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    c = tensor_case
    U0 = ost.initial_state(ost.build(c["om"].mesh))
    U_cpu = U0.copy()
    its_cpu, _ = newton_solve(c["om"], U_cpu, U0, U0, 5e-12, 1e30, 1e-8, 25)
    prob = wr.device_problem(c["mesh"].coords, c["mesh"].cells, wr.device_two_species_model())
    for split in (False, True):
        prob.set_state(U0, U0, U0)
        prob.set_step(5e-12, 1e30)
        if split:
            prob.setup_multigrid(**streamer.MULTIGRID)
            prob.set_fieldsplit(chebyshev_weights(6))
        its, _ = prob.newton_solve(rtol=1e-8, max_it=25, ksp_rtol=1e-10, ksp_max_it=2000)
        d = np.abs(prob.get_state() - U_cpu).max(axis=0) / np.abs(U_cpu).max(axis=0)
        print(f"[walls] newton split={split}: its {its} (restatement {its_cpu}) diff {d}", flush=True)
        assert its == its_cpu, (split, its, its_cpu)
        assert d.max() < 1e-8, (split, d)
    assert prob.launched_assembly()["jacobian"]["variant"] == "lds-patches"
    prob.close()


def test_species_only_assembly(tensor_case):
    """The species rows and J_uu of fedm_debug_species_assembly equal the coupled assembly's: a wall model takes the full
    second-generation assembly there (bounds of test_gpu_tabulated.py's species-only test)."""
    import segregated_reference as sr
    c = tensor_case
    U, Uo, Uo1 = c["states"]
    prob = wr.device_problem(c["mesh"].coords, c["mesh"].cells, wr.device_two_species_model())
    prob.set_state(U, Uo, Uo1)
    prob.set_step(*DT)
    prob.jacobian()
    F, J = prob.residual_vector(), prob.jacobian_csr()
    assert prob.species_assembly(jacobian=True) is False          # the full assembly, not the one-pass kernel
    Fs, Js = prob.residual_vector(), prob.jacobian_csr()
    prob.close()
    iu, ip = sr.block_indices(U.size, 3)
    assert np.all(Fs[ip] == 0.0)
    assert np.abs(Fs[iu] - F[iu]).max() <= 1e-12 * np.abs(F[iu]).max()
    Juu, Juu_s = sr.species_block(J, 3), sr.species_block(Js, 3)
    rowmax = abs(Juu).max(axis=1).toarray().ravel()
    assert (abs(Juu_s - Juu).max(axis=1).toarray().ravel() <= 1e-11 * rowmax + 1e-300).all()
    # ... and against the restatement, emission plane included
    assert _rel_rows(Juu_s, sr.species_block(c["J"], 3)) < 1e-10


def _raw_create(md, wd, mesh, creator="walls"):
    """fedm_ctx_create_walls (or one of the older creators) through the ABI; returns (rc, message, handle value)."""
    from fedm_amd import _lib
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Marking_boundaries
    lib = _lib.load()
    coords = np.ascontiguousarray(mesh.coords, dtype=np.float64)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int32)
    tags = np.ascontiguousarray(Marking_boundaries(mesh, streamer.BOUNDARIES), dtype=np.int8)
    dofs, vals = streamer.dirichlet(coords)
    if not md.poisson:
        dofs, vals = dofs[:0], vals[:0]
    mdesc = _lib.MeshDesc()
    mdesc.n_vertices, mdesc.n_cells = coords.shape[0], cells.shape[0]
    mdesc.coords = coords.ctypes.data_as(C.POINTER(C.c_double))
    mdesc.cells = cells.ctypes.data_as(C.POINTER(C.c_int32))
    mdesc.facet_tags = tags.ctypes.data_as(C.POINTER(C.c_int8))
    mdesc.n_dirichlet = dofs.size
    mdesc.dirichlet_dofs = dofs.ctypes.data_as(C.POINTER(C.c_int32))
    mdesc.dirichlet_vals = vals.ctypes.data_as(C.POINTER(C.c_double))
    handle = C.c_void_p()
    if creator == "walls":
        rc = lib.fedm_ctx_create_walls(C.byref(mdesc), C.byref(md), None if wd is None else C.byref(wd), 0, None, None,
                                       None, 0, C.byref(handle))
    elif creator == "tabulated":
        rc = lib.fedm_ctx_create_tabulated(C.byref(mdesc), C.byref(md), 0, None, None, None, 0, C.byref(handle))
    else:
        rc = lib.fedm_ctx_create(C.byref(mdesc), C.byref(md), 0, C.byref(handle))
    msg = _lib.last_error()
    if rc == 0:
        lib.fedm_ctx_destroy(handle)
    return rc, msg, handle.value


def test_refusals_through_the_abi(tensor_case):
    """Every refusal of fedm_ctx_create_walls: -2, a message that names the tag (and the species), no context -- and a
    valid creation works afterwards."""
    from fedm_amd.device import Model, Walls
    from fedm_amd.termsum import TermSum
    mesh = tensor_case["mesh"]
    model = wr.device_two_species_model()

    def desc(change=None, model=model):
        md, wd = model.to_c(), model.walls_to_c()
        if change:
            change(md, wd)
        return md, wd

    def setter(field, t, s, value):
        def change(md, wd):
            getattr(wd, field)[t][s] = value
        return change

    def gamma(t, value):
        def change(md, wd):
            wd.gamma[t] = value
        return change

    def drift_w(md, wd):
        md.has_drift_w[0] = 1

    def no_emitter(md, wd):
        wd.emits[1] = 0

    def gamma_on_a_tag_without_walls_is_ignored(md, wd):
        wd.gamma[2] = 0.5

    no_poisson = Model(n_species=1, poisson=False, eq_type=["drift-diffusion-reaction"], Z=[1.0],
                       mu=[TermSum.const(2e-4)], D=[TermSum.const(3e-6)], bc_kind=[["flux source"]] * 2 + [["zero flux"]] * 2,
                       quadrature_degree=2,
                       walls=Walls(vth=[[4e2]] * 4, ref=[[0.3]] * 4, gamma=[0.0] * 4, emits=[False], is_ion=[False]))
    cases = [("ref = -1", desc(setter("ref", 0, 1, -1.0)), "tag 1, species 1"),
             ("ref NaN", desc(setter("ref", 1, 0, np.nan)), "tag 2, species 0"),
             ("vth negative", desc(setter("vth", 0, 0, -1.0)), "tag 1, species 0"),
             ("vth infinite", desc(setter("vth", 1, 1, np.inf)), "tag 2, species 1"),
             ("gamma NaN", desc(gamma(1, np.nan)), "tag 2"),
             ("no Poisson equation", desc(model=no_poisson), "tag 1, species 0"),
             ("constant drift velocity", desc(drift_w), "tag 1, species 0"),
             ("gamma without an emitter", desc(no_emitter), "tag 1")]
    for name, (md, wd), expect in cases:
        rc, msg, h = _raw_create(md, wd, mesh)
        print(f"[walls] refusal {name}: {rc} {msg!r}", flush=True)
        assert rc == -2 and h is None and expect in msg and "fedm_ctx_create_walls" in msg, name
        rc, msg, h = _raw_create(*desc(), mesh)
        assert rc == 0, (name, msg)                       # a valid creation right after the refusal
    # the older creators are this call without walls: they refuse kind 2 with a message
    for creator in ("plain", "tabulated"):
        rc, msg, h = _raw_create(model.to_c(), None, mesh, creator=creator)
        print(f"[walls] refusal {creator} creator: {rc} {msg!r}", flush=True)
        assert rc == -2 and h is None and "tag 1, species 0" in msg and "fedm_ctx_create_walls" in msg
    rc, msg, h = _raw_create(model.to_c(), None, mesh)    # the new creator without a wall description
    assert rc == -2 and h is None and "tag 1, species 0" in msg
    rc, msg, h = _raw_create(*desc(gamma_on_a_tag_without_walls_is_ignored), mesh)
    assert rc == 0, msg
