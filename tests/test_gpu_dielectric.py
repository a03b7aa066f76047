"""Dielectric layers of LFA models on the device against the numpy restatement (tests/dielectric_reference.py).

The wall model of tests/test_gpu_wall_flux.py with a layer on the cathode (tag 1: both species 'flux source', the
electrons with secondary emission; the electrode's Dirichlet values leave with it, the conductor is behind the layer)
or on r = BOX (tag 4: the electrons' Neumann term; the corner vertices there are on the layer and on a Dirichlet
electrode).  States, step pair and bounds are those of test_gpu_wall_flux.py; F and the product are held to them per
component, so that the Poisson row counts on its own scale (next to the species rows' 1e18 it would not count at all),
and the Poisson rows of the layer vertices to BOUND_J_LAYER besides (tests/test_dielectric_reference.py derives it
and shows what each bound would catch).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import dielectric_reference as dr
import wall_flux_reference as wr
from test_dielectric_reference import (BOUND_F, BOUND_J, BOUND_J_LAYER, BOUND_P, BOUND_Q, CONSERVATION_BC, ChargeLedger,
                                       component_error, conservation_case, layer_row_error, row_error)
from test_gpu_wall_flux import DT, PATHS

pytestmark = pytest.mark.gpu


def _case(coords, cells, config, **model_kw):
    """Mesh, restatement with a random charge history, states and the restatement's F and J (computed once)."""
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.mesh import Mesh
    msh = Mesh(coords, cells)
    om = dr.oracle_two_species(OMesh(msh.coords, msh.cells), config, **model_kw)
    log = model_kw.get("log", True)
    U = wr.wall_state(msh.coords, log=log)
    wr.assert_preconditions(om, U)
    rng = np.random.default_rng(3)
    if log:
        Uo, Uo1 = U - 0.01 * rng.random(U.shape), U - 0.02 * rng.random(U.shape)
    else:
        Uo, Uo1 = U * (1.0 - 0.01 * rng.random(U.shape)), U * (1.0 - 0.02 * rng.random(U.shape))
    om.q, om.q_old = dr.random_history(om)
    F, J = om.residual_jacobian(U, Uo, Uo1, *DT)
    return dict(mesh=msh, om=om, config=config, states=(U, Uo, Uo1), F=F, J=J)


_MESHES = {}


def _mesh(name):
    if name not in _MESHES:
        from fedm_amd.cases import streamer
        if name == "tensor":
            m = streamer.mesh(20, 2.0)
            _MESHES[name] = (m.coords, m.cells)
        elif name == "unstructured":
            m = streamer.refined_mesh(60e-6)
            _MESHES[name] = (m.coords, m.cells)
        else:            # 140 tagged facets: two 128-thread facet blocks, the second partial
            import limit_meshes
            _MESHES[name] = limit_meshes.build("cells192")
    return _MESHES[name]


_CASES = {}


def case(mesh, config):
    if (mesh, config) not in _CASES:
        _CASES[mesh, config] = _case(*_mesh(mesh), config)
    return _CASES[mesh, config]


def _against_the_restatement(prob, c, what, expect_variant=None):
    om, (U, Uo, Uo1) = c["om"], c["states"]
    F_cpu, J_cpu, neq = c["F"], c["J"], om.neq
    prob.set_state(U, Uo, Uo1)
    prob.set_step(*DT)
    prob.set_dielectric_charge(om.q, om.q_old)
    F_gpu, fnorm = prob.residual()
    eF = component_error(F_gpu, F_cpu, neq)
    eJ, eL = [], []
    for _ in range(2):      # twice in a row: a plane that is kept although the facets add to it shows on the second one
        prob.jacobian()
        J_gpu = prob.jacobian_csr()
        eJ.append(row_error(J_gpu, J_cpu))
        eL.append(layer_row_error(J_gpu, J_cpu, om))
    launched = prob.launched_assembly()
    xv = np.random.default_rng(5).normal(size=prob.n)
    eP = component_error(prob.spmv(xv), J_cpu @ xv, neq)
    print(f"[dielectric] {what}: F {eF:.2e} J {eJ[0]:.2e} {eJ[1]:.2e} layer rows {eL[0]:.2e} {eL[1]:.2e} product {eP:.2e} "
          f"launched {launched}", flush=True)
    for kind in ("residual", "jacobian"):
        assert launched[kind]["variant"] != "lds-patches/one-pass"
        if expect_variant is not None:
            assert launched[kind]["variant"] == expect_variant
    assert eF < BOUND_F
    assert fnorm == pytest.approx(np.linalg.norm(F_cpu), rel=1e-11)
    assert max(eJ) < BOUND_J
    assert max(eL) < BOUND_J_LAYER
    assert eP < BOUND_P


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("config", list(dr.CONFIGS))
@pytest.mark.parametrize("mesh", ["tensor", "unstructured", "cells192"])
def test_against_the_restatement(mesh, config, path, monkeypatch):
    c = case(mesh, config)
    if mesh == "cells192":
        assert (c["om"].facet_tags > 0).sum() == 140
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    prob = dr.device_problem(c["mesh"].coords, c["mesh"].cells, dr.device_two_species_model(config), config)
    expect = None if mesh == "cells192" else ("lds-patches" if path == "default" else path)
    try:
        _against_the_restatement(prob, c, f"{mesh} {config} {path}", expect)
    finally:
        prob.close()


def test_corner_vertex_keeps_its_dirichlet_row():
    """(r, z) = (BOX, 0) and (BOX, BOX) are on the layer of r = BOX and Dirichlet vertices of the potential: F = u - g
    and the unit row there, and q_a -- which the row no longer sees -- as the restatement accepts it."""
    from fedm_amd.cases import streamer
    c = case("tensor", "outer")
    om, (U, Uo, Uo1) = c["om"], c["states"]
    corners = np.intersect1d(om.layer_vertices * 3 + 2, om.dirichlet_dofs)
    assert corners.size == 2
    prob = dr.device_problem(c["mesh"].coords, c["mesh"].cells, dr.device_two_species_model("outer"), "outer")
    try:
        prob.set_state(U, Uo, Uo1)
        prob.set_step(*DT)
        prob.set_dielectric_charge(om.q, om.q_old)
        prob.jacobian()
        F, J = prob.residual_vector(), prob.jacobian_csr()
        vals = dict(zip(om.dirichlet_dofs, om.dirichlet_vals))
        for dof in corners:
            assert F[dof] == U.ravel()[dof] - vals[dof]
            row = J[dof].tocoo()
            assert dict(zip(row.col[row.data != 0.0], row.data[row.data != 0.0])) == {dof: 1.0}
        prob.dielectric_accept()
        q_gpu = prob.dielectric_charge()["q"]
        q_cpu = om.charge(U, *DT)
        assert np.abs(q_cpu[corners // 3]).min() > 0.0
        assert np.abs(q_gpu - q_cpu)[corners // 3].max() <= BOUND_Q * np.abs(q_cpu).max()
    finally:
        prob.close()


def test_linear_representation():
    coords, cells = _mesh("tensor")
    c = _case(coords, cells, "cathode", log=False)
    prob = dr.device_problem(coords, cells, dr.device_two_species_model("cathode", log=False), "cathode")
    try:
        _against_the_restatement(prob, c, "linear representation")
    finally:
        prob.close()


def test_tabulated_coefficients():
    import tabulated_reference as tr
    from fedm_amd.termsum import TermSum
    c0 = case("tensor", "cathode")
    coords, cells = _mesh("tensor")
    Em = c0["om"].cell_fields(c0["states"][0])[2]
    x = tr.quantile_knots(Em)
    mu_y, D_y, _ = tr.closed_forms(x)
    one = [(1.0, 0.0, 0.0, 0.0)]
    c = _case(coords, cells, "cathode", mu_e=tr.TabulatedTermSum(one, [(x, mu_y)]), D_e=tr.TabulatedTermSum(one, [(x, D_y)]))
    model = dr.device_two_species_model("cathode", mu_e=TermSum.table(x, mu_y), D_e=TermSum.table(x, D_y))
    prob = dr.device_problem(coords, cells, model, "cathode")
    try:
        _against_the_restatement(prob, c, "tabulated mu_e, D_e", "lds-patches")
    finally:
        prob.close()


def test_four_species():
    """tests/lfa_models.py's four-species model with the walls of the wall tests and the layer on the cathode."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import Dielectric, DeviceProblem
    from fedm_amd.mesh import Marking_boundaries
    m, model, om0, ddofs, dvals = wr.four_species_pair()
    keep = np.abs(m.coords[ddofs // 5, 1]) > 3e-16          # the cathode's values leave with the electrode
    ddofs, dvals = ddofs[keep], dvals[keep]
    om = dr.with_layers(om0, dr.layers_of("cathode"))
    om.set_dirichlet(ddofs, dvals)
    model.dielectric = Dielectric(thickness={1: dr.LAYER_D}, eps_r={1: dr.LAYER_EPS_R}, voltage={1: dr.LAYER_U})
    U = wr.wall_state(m.coords, neq=5)
    U.ravel()[ddofs] = dvals
    wr.assert_preconditions(om, U)
    rng = np.random.default_rng(4)
    Uo, Uo1 = U - 0.01 * rng.random(U.shape), U - 0.02 * rng.random(U.shape)
    om.q, om.q_old = dr.random_history(om)
    F, J = om.residual_jacobian(U, Uo, Uo1, *DT)
    prob = DeviceProblem(m.coords, m.cells, model, facet_tags=Marking_boundaries(m, streamer.BOUNDARIES),
                         dirichlet_dofs=ddofs.astype(np.int32), dirichlet_vals=dvals)
    try:
        _against_the_restatement(prob, dict(om=om, states=(U, Uo, Uo1), F=F, J=J), "four species")
    finally:
        prob.close()


def _planar_divider_problem(n=12):
    """The CPU test's divider on the device: planar, a layer on z = 0, V on z = g, no charge."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import Dielectric, DeviceProblem, Model
    from fedm_amd.mesh import Marking_boundaries
    from fedm_amd.termsum import TermSum, parse
    msh = streamer.mesh(n)
    g, V, U_l, d, eps_r = streamer.BOX, 1000.0, 100.0, 2e-4, 5.0
    model = Model(n_species=2, poisson=True, eq_type=["drift-diffusion-reaction"] * 2, Z=[1.0, -1.0],
                  mu=[TermSum.const(wr.MU_ION), parse(streamer.MU_E)], D=[TermSum.const(wr.D_ION), parse(streamer.D_E)],
                  bc_kind=[["zero flux"] * 2] * 4, quadrature_degree=2, axisymmetric=False,
                  dielectric=Dielectric(thickness={1: d}, eps_r={1: eps_r}, voltage={1: U_l}))
    top = np.nonzero(np.abs(msh.coords[:, 1] - g) < 3e-16)[0]
    prob = DeviceProblem(msh.coords, msh.cells, model, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                         dirichlet_dofs=(top * 3 + 2).astype(np.int32), dirichlet_vals=np.full(top.size, V))
    U = np.full((msh.coords.shape[0], 3), -200.0)
    U[:, 2] = V * msh.coords[:, 1] / g + 1.0
    prob.set_state(U, U, U)
    prob.set_step(1e-12, 1e30)
    expect = U_l + (V - U_l) * (d / eps_r) / (g + d / eps_r)
    return prob, msh, expect, (g, V, U_l, d, eps_r)


def test_poisson_only_jacobian_and_the_divider():
    """fedm_jacobian_poisson_only: the Laplacian and the Robin mass term, nothing of the mirror (whose potential column
    the coupled Jacobian of the same state does hold); the hierarchy built from it and fedm_poisson_solve give the
    series-capacitor divider."""
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.cases import streamer
    c = case("tensor", "cathode")
    om, (U, Uo, Uo1) = c["om"], c["states"]
    prob = dr.device_problem(c["mesh"].coords, c["mesh"].cells, dr.device_two_species_model("cathode"), "cathode")
    try:
        prob.set_state(U, Uo, Uo1)
        prob.set_step(*DT)
        prob._check(prob.lib.fedm_jacobian_poisson_only(prob._h), "fedm_jacobian_poisson_only")
        K = sp.csr_matrix(prob.block_csr(2, 2))[prob._inv][:, prob._inv]       # device numbering -> the caller's
    finally:
        prob.close()
    plain = wr.oracle_two_species(OMesh(c["mesh"].coords, c["mesh"].cells))
    _, Jp = plain.residual_jacobian(U, Uo, Uo1, *DT, apply_bc=False)
    K_ref = (Jp[2::3][:, 2::3] + om.robin_matrix()).tocsr()
    free = np.setdiff1d(np.arange(K.shape[0]), om.dirichlet_dofs // 3)
    layer = np.setdiff1d(om.layer_vertices, om.dirichlet_dofs // 3)
    e = row_error(K[free], K_ref[free])
    mirror = row_error(c["J"][2::3][:, 2::3][layer], K_ref[layer])
    print(f"[dielectric] Poisson-only (Phi, Phi): {e:.2e} from Laplacian + Robin; the coupled block is {mirror:.2e} away", flush=True)
    assert abs(om.robin_matrix()).max() > 0.0
    assert e < BOUND_J_LAYER < 1e-2 * mirror
    # the divider
    prob, msh, expect, (g, V, U_l, d, eps_r) = _planar_divider_problem()
    try:
        prob.setup_multigrid(**streamer.MULTIGRID)
        prob.poisson_solve(rtol=1e-12)
        phi = prob.get_state()[:, 2]
        bottom = np.abs(msh.coords[:, 1]) < 3e-16
        err = np.abs(phi[bottom] - expect).max() / V
        disp = prob.dielectric_charge()["displacement"][1]
        print(f"[dielectric] divider on the device: error {err:.2e}, displacement charge {disp:.6e}", flush=True)
        assert err < 1e-9             # the CG's rtol times the condition of a 12 x 12 Laplacian (~1e2), not rounding
        assert disp == pytest.approx(8.854187817e-12 * eps_r / d * (expect - U_l) * g, rel=1e-9)
    finally:
        prob.close()


def test_accept_and_reproducible_totals():
    """After a state shift the accept gives the restatement's q and q_old to 1e-12 of max |q|; the totals are the
    restatement's sums; two dielectric_charge() calls return the same bytes, and so does a second run of it all."""
    import copy
    runs = []
    for config in dr.CONFIGS:
        c = case("unstructured", config)
        om, (U, Uo, Uo1) = copy.copy(c["om"]), c["states"]
        tag = dr.CONFIGS[config]
        for _ in range(2):
            prob = dr.device_problem(c["mesh"].coords, c["mesh"].cells, dr.device_two_species_model(config), config)
            try:
                prob.set_state(U, Uo, Uo1)
                prob.set_step(*DT)
                prob.set_dielectric_charge(om.q, om.q_old)
                prob.shift_state()
                prob.dielectric_accept()
                a, b = prob.dielectric_charge(), prob.dielectric_charge()
            finally:
                prob.close()
            assert all(np.array_equal(a[k], b[k]) for k in ("q", "q_old")) and a["charge"] == b["charge"] \
                and a["displacement"] == b["displacement"]
            runs.append(a)
        assert np.array_equal(runs[-1]["q"], runs[-2]["q"]) and runs[-1]["charge"] == runs[-2]["charge"]
        q_cpu = om.charge(U, *DT)
        eq = np.abs(a["q"] - q_cpu).max() / np.abs(q_cpu).max()
        eo = np.abs(a["q_old"] - om.q).max() / np.abs(q_cpu).max()
        print(f"[dielectric] accept {config}: q {eq:.2e} q_old {eo:.2e}; charge {a['charge'][tag]:.6e} C, displacement "
              f"{a['displacement'][tag]:.6e} C on {a['n_layer_vertices']} vertices", flush=True)
        assert eq <= BOUND_Q and eo == 0.0
        assert a["n_layer_vertices"] == om.layer_vertices.size
        assert a["charge"][tag] == pytest.approx(q_cpu.sum(), rel=1e-12, abs=1e-12 * np.abs(q_cpu).sum())
        assert a["displacement"][tag] == pytest.approx(om.displacement_charge(U)[tag], rel=1e-11)


def _raw_create(md, wd, dd, mesh, n_owned=None):
    """fedm_ctx_create_dielectric through the ABI; returns (rc, message, handle value)."""
    from fedm_amd import _lib
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Marking_boundaries
    lib = _lib.load()
    coords = np.ascontiguousarray(mesh.coords, dtype=np.float64)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int32)
    tags = np.ascontiguousarray(Marking_boundaries(mesh, streamer.BOUNDARIES), dtype=np.int8)
    mdesc = _lib.MeshDesc()
    mdesc.n_vertices, mdesc.n_cells = coords.shape[0], cells.shape[0]
    mdesc.coords = coords.ctypes.data_as(C.POINTER(C.c_double))
    mdesc.cells = cells.ctypes.data_as(C.POINTER(C.c_int32))
    mdesc.facet_tags = tags.ctypes.data_as(C.POINTER(C.c_int8))
    if n_owned is not None:
        mdesc.n_owned_vertices = n_owned
    handle = C.c_void_p()
    rc = lib.fedm_ctx_create_dielectric(C.byref(mdesc), C.byref(md), None if wd is None else C.byref(wd),
                                        None if dd is None else C.byref(dd), 0, None, None, None, 0, C.byref(handle))
    msg = _lib.last_error()
    if rc == 0:
        lib.fedm_ctx_destroy(handle)
    return rc, msg, handle.value


def test_refusals_through_the_abi():
    """Every refusal: -2, a message that says why and names the tag, no context; a valid creation right after."""
    import lmea_models as lm
    from fedm_amd import _lib
    from fedm_amd.device import DeviceProblem, Model, Walls
    from fedm_amd.termsum import TermSum
    mesh = case("tensor", "cathode")["mesh"]
    model = dr.device_two_species_model("cathode")

    def desc(change=None, model=model):
        md, wd, dd = model.to_c(), model.walls_to_c(), model.dielectric.to_c()
        if change:
            change(dd)
        return md, wd, dd

    def setter(field, value):
        def change(dd):
            getattr(dd, field)[0] = value
        return change

    no_poisson = Model(n_species=1, poisson=False, eq_type=["drift-diffusion-reaction"], Z=[1.0], mu=[TermSum.const(2e-4)],
                       D=[TermSum.const(3e-6)], bc_kind=[["zero flux"]] * 4, quadrature_degree=2, dielectric=model.dielectric)
    cases = [("no Poisson equation", desc(model=no_poisson), {}, "no Poisson equation"),
             ("ghost vertices", desc(), dict(n_owned=mesh.coords.shape[0] - 5), "ghost vertices"),
             ("d = 0", desc(setter("thickness", 0.0)), {}, "thickness"),
             ("d negative", desc(setter("thickness", -1e-4)), {}, "thickness"),
             ("d NaN", desc(setter("thickness", np.nan)), {}, "thickness"),
             ("eps_r = 0", desc(setter("eps_r", 0.0)), {}, "permittivity"),
             ("eps_r negative", desc(setter("eps_r", -2.0)), {}, "permittivity")]
    for name, (md, wd, dd), kw, expect in cases:
        rc, msg, h = _raw_create(md, wd, dd, mesh, **kw)
        print(f"[dielectric] refusal {name}: {rc} {msg!r}", flush=True)
        assert rc == -2 and h is None and expect in msg and "tag 1" in msg and "fedm_ctx_create_dielectric" in msg, name
        rc, msg, h = _raw_create(*desc(), mesh)
        assert rc == 0, (name, msg)
    # a layer on an LMEA context: its creator takes none, and the layer calls refuse the context
    lib = _lib.load()
    c = lm.case("e-only", "3x3")
    gd = DeviceProblem(c.mesh.coords, c.mesh.cells, c.model, facet_tags=c.mesh.tags, dirichlet_dofs=c.dirichlet_dofs,
                       dirichlet_vals=c.dirichlet_vals)
    try:
        U8 = (C.c_double * _lib.MAX_TAGS)()
        for call in (lambda: lib.fedm_dielectric_accept(gd._h), lambda: lib.fedm_dielectric_set_voltage(gd._h, U8),
                     lambda: lib.fedm_dielectric_get(gd._h, None, None, None), lambda: lib.fedm_dielectric_set(gd._h, None, None)):
            assert call() == -2 and "LMEA" in _lib.last_error()
    finally:
        gd.close()
    # ... a context without a layer, and the segregated step on one with a layer
    plain = wr.device_problem(mesh.coords, mesh.cells, wr.device_two_species_model())
    try:
        assert lib.fedm_dielectric_accept(plain._h) == -2 and "no dielectric layer" in _lib.last_error()
    finally:
        plain.close()
    prob = dr.device_problem(mesh.coords, mesh.cells, model, "cathode")
    try:
        with pytest.raises(RuntimeError, match="dielectric layer"):
            prob.poisson_update()
        with pytest.raises(RuntimeError, match="not finite"):
            prob.set_layer_voltage({1: np.inf})
        prob.set_layer_voltage({1: 12.0})
        assert prob.dielectric_charge(vertices=False)["voltage"] == {1: 12.0}
    finally:
        prob.close()


def test_a_layer_free_model_is_the_context_it_was(monkeypatch):
    """fedm_ctx_create_dielectric without a layer beside fedm_ctx_create_walls: F, J and launched_assembly() byte for
    byte (global colouring: the assembly with a fixed summation order)."""
    from fedm_amd.device import Dielectric
    monkeypatch.setenv("FEDM_ASSEMBLY", "colour")
    c = case("tensor", "cathode")
    U, Uo, Uo1 = c["states"]
    out = []
    for layered in (False, True):
        model = wr.device_two_species_model()
        if layered:
            model.dielectric = Dielectric(thickness={})
        prob = wr.device_problem(c["mesh"].coords, c["mesh"].cells, model)
        try:
            prob.set_state(U, Uo, Uo1)
            prob.set_step(*DT)
            prob.jacobian()
            J = prob.jacobian_csr()
            out.append((prob.residual_vector().tobytes(), J.indptr.tobytes(), J.indices.tobytes(), J.data.tobytes(),
                        prob.launched_assembly(), prob.plane_masks()))
        finally:
            prob.close()
    assert out[0] == out[1]


def test_newton_steps_against_the_restatement():
    """Three Newton-solved steps with the field split and the multigrid cycle against the restatement's dense Newton,
    the accept after each: iteration counts and 1e-8 as test_gpu_wall_flux.py's test_newton_step_against_the_restatement,
    and the accepted q to the same 1e-8 of max |q| (it is a function of the solved state).  The model is the
    logarithmic one, whose time term n BDF2(u) conserves no charge discretely, with or without a layer: the conservation
    bound is held where it holds, in the linear representation (tests/test_dielectric_reference.py); here the device's
    plasma state and surface charge follow the restatement's; test_charge_conservation_on_the_device holds the device
    to the bound itself."""
    from oracle import streamer as ost
    from oracle.newton import newton_solve
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    import copy
    c = case("tensor", "cathode")
    om = copy.copy(c["om"])
    om.q, om.q_old = np.zeros_like(om.q), np.zeros_like(om.q)
    U0 = ost.initial_state(ost.build(om.mesh))
    prob = dr.device_problem(c["mesh"].coords, c["mesh"].cells, dr.device_two_species_model("cathode"), "cathode")
    try:
        prob.set_state(U0, U0, U0)
        prob.setup_multigrid(**streamer.MULTIGRID)
        prob.set_fieldsplit(chebyshev_weights(6))
        U, Uo, Uo1, dt_old = U0.copy(), U0.copy(), U0.copy(), 1e30
        for dt in (5e-12, 4e-12, 6e-12):
            its_cpu, _ = newton_solve(om, U, Uo, Uo1, dt, dt_old, 1e-8, 25)
            om.accept(U, dt, dt_old)
            prob.set_step(dt, dt_old)
            its, _ = prob.newton_solve(rtol=1e-8, max_it=25, ksp_rtol=1e-10, ksp_max_it=2000)
            prob.shift_state()
            prob.dielectric_accept()
            got = prob.dielectric_charge()
            d = np.abs(prob.get_state() - U).max(axis=0) / np.abs(U).max(axis=0)
            eq = np.abs(got["q"] - om.q).max() / np.abs(om.q).max()
            print(f"[dielectric] newton dt {dt}: its {its} (restatement {its_cpu}) diff {d} q {eq:.2e} "
                  f"charge {got['charge'][1]:.4e} C", flush=True)
            assert its == its_cpu, (dt, its, its_cpu)
            assert d.max() < 1e-8 and eq < 1e-8
            Uo1, Uo, dt_old = Uo, U.copy(), dt
        assert prob.launched_assembly()["jacobian"]["variant"] == "lds-patches"
    finally:
        prob.close()


def test_charge_conservation_on_the_device():
    """Three Newton-solved steps with unequal dt, field split and multigrid cycle, in the representation in which the
    scheme conserves (the linear one; tests/test_dielectric_reference.py, test_charge_conservation and ChargeLedger):
    the layer on the cathode is the only boundary with a species flux.  The plasma charge e sum_s Z_s N_s of the
    downloaded state plus the surface charge of dielectric_charge() stays within the CPU test's bound -- the
    restatement's species residual at the device's own states, times the same 1.5, plus the same rounding term."""
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    from fedm_amd.mesh import Mesh
    coords, cells = _mesh("tensor")
    msh = Mesh(coords, cells)
    om, U0 = conservation_case(OMesh(msh.coords, msh.cells))
    model = dr.device_two_species_model("cathode", log=False)
    model.bc_kind = CONSERVATION_BC
    prob = dr.device_problem(msh.coords, msh.cells, model, "cathode")
    try:
        prob.set_state(U0, U0, U0)
        prob.setup_multigrid(**streamer.MULTIGRID)
        prob.set_fieldsplit(chebyshev_weights(6))
        ledger = ChargeLedger(om, U0, np.zeros(msh.coords.shape[0]))
        Uo, Uo1, dt_old = U0.copy(), U0.copy(), 1e30
        for dt in (2e-12, 3e-12, 2.5e-12):
            prob.set_step(dt, dt_old)
            its, _ = prob.newton_solve(rtol=1e-10, max_it=25, ksp_rtol=1e-10, ksp_max_it=2000)
            prob.shift_state()
            prob.dielectric_accept()
            U, got = prob.get_state(), prob.dielectric_charge()
            assert got["charge"][1] == pytest.approx(got["q"].sum(), rel=1e-12)
            ledger.step(U, Uo, Uo1, dt, dt_old, got["q"])
            print(f"[dielectric] device step dt {dt}: {its} Newton iterations, drift {ledger.drift[-1]:.3e} C", flush=True)
            Uo1, Uo, dt_old = Uo, U.copy(), dt
        ledger.check("device", got["q"])
    finally:
        prob.close()


def test_stepper_accepts_after_its_shift():
    """Two Stepper steps with a coated cathode: the accept rides on the state shift (or on surface_charge(), whichever
    comes first, once), so the charge is there after the first step, has grown after the second, and a second reading
    changes nothing; snapshot and restore carry the charge."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import Dielectric
    msh = streamer.mesh(20, 2.0)
    layer = Dielectric(thickness={1: 1e-4}, eps_r={1: 4.0})
    prob = streamer.device_problem(msh.coords, msh.cells, dielectric=layer)
    try:
        assert layer.voltage == {} and prob.model.dielectric.voltage == {1: 0.0}       # the caller's description is a copy
        stp = streamer.Stepper(prob)
        stp.initialise()
        assert stp.surface_charge()["charge"][1] == 0.0
        stp.step()
        q1 = stp.surface_charge()["charge"][1]
        snap = stp.snapshot()
        stp.step()
        behind_the_shift = prob.dielectric_charge(vertices=False)["charge"][1]     # step 1's, accepted by step 2's shift
        q2 = stp.surface_charge()["charge"][1]
        print(f"[dielectric] stepper: surface charge {q1:.4e} C after one step, {q2:.4e} C after two", flush=True)
        assert q1 != 0.0 and behind_the_shift == q1 and abs(q2) > abs(q1)
        assert stp.surface_charge()["charge"][1] == q2
        stp.restore(snap)
        assert prob.dielectric_charge(vertices=False)["charge"][1] == q1
        stp.step()
        assert stp.surface_charge()["charge"][1] == pytest.approx(q2, rel=1e-9)
        assert prob.launched_assembly()["jacobian"]["variant"] == "lds-patches"
    finally:
        prob.close()


def test_the_example_runs_with_a_coated_cathode(tmp_path):
    """examples/streamer_discharge.py --dielectric 1:1e-4:4 --surface-charge-log FILE: the facade's time loop
    (adaptive_solver, the accept behind the Functions' state shift) writes a charge that grows step by step."""
    import importlib.util
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("streamer_example_dielectric", root / "examples" / "streamer_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    log = tmp_path / "charge.log"
    state, _ = mod.main(cells=24, end_time=1.5e-11, output_dir=tmp_path, quiet=True, dielectric="1:1e-4:4",
                        surface_charge_log=str(log))
    rows = np.loadtxt(log, ndmin=2)
    print(f"[dielectric] example: {rows.shape[0]} rows, surface charge {rows[:, 1]}", flush=True)
    assert rows.shape[0] >= 2 and rows.shape[1] == len(mod.SURFACE_CHARGE_COLUMNS)
    assert np.isfinite(state).all() and (np.abs(np.diff(rows[:, 1])) > 0).all() and rows[0, 1] != 0.0
    assert (rows[:, 3] == 0.0).all() and (rows[:, 2] != 0.0).all()
