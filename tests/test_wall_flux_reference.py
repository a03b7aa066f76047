"""'flux source' walls of LFA models without a GPU: the numpy restatement the GPU tests compare against
(tests/wall_flux_reference.py) checked by hand and against its own finite differences, and the façade's lowering of
Boundary_flux('flux source', ...) onto fedm_model_desc + fedm_wall_desc.
"""
import numpy as np
import pytest

import wall_flux_reference as wr


# ---- 1. one facet by hand -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.0, 0.07])
@pytest.mark.parametrize("ref", [0.0, 0.5])
@pytest.mark.parametrize("pz", [2.0e6, -1.5e6])
def test_one_facet_by_hand(pz, ref, gamma):
    """One cell with its facet A-B on z = 0 (outward normal (0, -1)), uniform log densities, Phi = 7 + px r + pz z:
    E = (-px, -pz), E.n = pz, grad(n) = 0, so the wall flux density g is one number per species and
    R[a][s] = 2 pi g int_AB phi_a r ds = 2 pi g L (r_a / 3 + r_b / 6)."""
    from oracle.mesh import Mesh as OMesh
    coords = np.array([[0.002, 0.0], [0.005, 0.0], [0.003, 0.004]])
    mesh = OMesh(coords, np.array([[0, 1, 2]]))
    tags = np.array([[0, 0, wr.CATHODE]], dtype=np.int8)          # the facet opposite vertex 2
    walls = wr.two_species_walls()
    walls["ref"][wr.CATHODE - 1] = [ref, ref]
    walls["gamma"][wr.CATHODE - 1] = gamma
    from oracle import streamer as ost
    om = wr.WallLFAModel(mesh, 2, True, ["drift-diffusion-reaction"] * 2, [1.0, -1.0], mu=[wr.MU_ION, ost.MU_E],
                         D=[wr.D_ION, ost.D_E], reactions=[(ost.K_ION, [0, 1], [1, 1])], facet_tags=tags,
                         bc_type=wr.WALL_BC, qdeg=2, walls=walls)
    px = 4.0e5
    ui, ue = np.log(3e15), np.log(2e14)
    U = np.column_stack([np.full(3, ui), np.full(3, ue), 7.0 + px * coords[:, 0] + pz * coords[:, 1]])
    Uc, E, Em = om.cell_fields(U)
    dEm = -np.einsum("cd,cbd->cb", E, om.G) / Em[:, None]
    Re = np.zeros((1, 3, 3))
    om._boundary(Uc, E, Em, dEm, [m(Em) for m in om.mu], Re, None)
    # the closed form
    En, Emag = pz, np.hypot(px, pz)
    fac = (1.0 - ref) / (1.0 + ref)
    n_i, n_e = 3e15, 2e14
    g_i = fac * (0.5 * wr.VTH_ION + abs(wr.MU_ION * En)) * n_i
    mu_e = 2.3987 * Emag ** -0.26
    g_e = fac * (0.5 * wr.VTH_E + abs(-mu_e * En)) * n_e - 2.0 * gamma / (1.0 + ref) * max(wr.MU_ION * En * n_i, 0.0)
    rA, rB, L = 0.002, 0.005, 0.003
    shape = 2.0 * np.pi * L * np.array([rA / 3.0 + rB / 6.0, rA / 6.0 + rB / 3.0])
    for s, g in ((0, g_i), (1, g_e)):
        assert np.abs(Re[0, :2, s] - g * shape).max() <= 1e-13 * np.abs(g * shape).max(), (s, Re[0, :, s], g * shape)
    assert np.all(Re[0, 2, :] == 0.0) and np.all(Re[0, :, 2] == 0.0)
    if gamma and pz > 0:          # the emission term is there, and only when the ions flow to the wall
        assert g_e != fac * (0.5 * wr.VTH_E + abs(mu_e * En)) * n_e


# ---- 2. the restatement's Jacobian against central differences of its own residual ----------------------------------
@pytest.fixture(scope="module")
def tensor_restatement():
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.cases import streamer
    msh = streamer.mesh(20, 2.0)
    om = wr.set_dirichlet(wr.oracle_two_species(OMesh(msh.coords, msh.cells)), msh.coords)
    U = wr.wall_state(msh.coords)
    return msh, om, U


def test_preconditions_hold_on_the_tensor_mesh(tensor_restatement):
    msh, om, U = tensor_restatement
    info = wr.assert_preconditions(om, U)
    assert info["tags"] == [wr.CATHODE, wr.ANODE] and info["n_facets"] == 40
    print(f"[walls] preconditions: {info}")


def _direction(coords, U_shape, seed=11):
    """A random direction scaled per field: N(0, 1) per node in the log densities; in the potential a random combination
    of smooth modes with maximum V0.  Nodal noise in the potential is no admissible direction at these steps: between
    the two rows of vertices at a wall (BOX / 20 apart) a change of h V0 N(0, 1) per node changes E.n by about
    h V0 sqrt(2) 20 / BOX = 4e4 V/m at h = 1e-3, more than |E.n| of the facet nearest to a sign change (2e4 V/m:
    |E.n| / |E| = 0.013), so U + h d and U - h d would lie on different branches of |E.n| and no difference quotient
    converges.  The modes below change E.n by at most h V0 4 pi / BOX = 1.9e4 V/m times coefficients well below 1;
    that every facet and facet point keeps its branch is asserted on the restatement's numbers, not assumed."""
    from fedm_amd.cases import streamer
    rng = np.random.default_rng(seed)
    d = rng.normal(size=U_shape)
    r, z = coords[:, 0] / streamer.BOX, coords[:, 1] / streamer.BOX
    phi = np.zeros(coords.shape[0])
    for k in range(1, 5):
        c, a, b = rng.normal() / k, rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        phi += c * np.sin(0.5 * k * np.pi * r + a) * np.cos(0.5 * k * np.pi * z + b)
    d[:, -1] = streamer.U_W * phi / np.abs(phi).max()
    return d


def test_jacobian_against_central_differences(tensor_restatement):
    """|(F(U + h d) - F(U - h d)) / 2h - J d| on the rows of the wall vertices falls as h^2: a missing or mis-signed
    term leaves an O(1) error that does not shrink."""
    from fedm_amd.cases import streamer
    msh, om, U = tensor_restatement
    z = msh.coords[:, 1]
    wall = np.nonzero((np.abs(z) < 1e-12) | (np.abs(z - streamer.BOX) < 1e-12))[0]
    rows = (wall[:, None] * 3 + np.arange(3)[None, :]).ravel()
    d = _direction(msh.coords, U.shape)
    dt, dto = 5e-12, 4e-12
    Uo, Uo1 = U - 0.01, U - 0.02
    _, J = om.residual_jacobian(U, Uo, Uo1, dt, dto)
    Jd = (J @ d.ravel())[rows]
    facets, points = om.diagnostics(U)
    err = []
    for h in (1e-3, 5e-4):
        for sign in (1.0, -1.0):          # the perturbed states stay on the branches of U
            f2, p2 = om.diagnostics(U + sign * h * d)
            assert all((a[1] > 0) == (b[1] > 0) for a, b in zip(facets, f2))
            assert all((a[1] + a[2] > 0) == (b[1] + b[2] > 0) for a, b in zip(points, p2))
        fd = (om.residual(U + h * d, Uo, Uo1, dt, dto) - om.residual(U - h * d, Uo, Uo1, dt, dto)) / (2.0 * h)
        err.append(np.abs(fd[rows] - Jd).max())
    print(f"[walls] central differences: err(1e-3) {err[0]:.3e} err(5e-4) {err[1]:.3e} |J d| {np.abs(Jd).max():.3e}")
    assert err[1] < 0.3 * err[0]
    assert err[1] < 1e-5 * np.abs(Jd).max()


# ---- 3. the façade --------------------------------------------------------------------------------------------------
def _wall_forms(mesh, vth_e=wr.VTH_E, mu_wall_e=None, ion_flux="sum", gamma=0.07):
    """A script-shaped LFA form: ions and electrons (both drift-diffusion) plus Poisson, 'flux source' on tag 1 (z = 0) for both
    species with Ion_flux = Max(dot(Gamma_ion, normal), 0), Neumann for the electrons on tag 4."""
    from fedm_amd import forms, functions as ff
    from fedm_amd.forms import (Expression, FacetNormal, FiniteElement, Function, FunctionSpace, Measure, MixedElement,
                                TestFunctions, TrialFunction, dot, dx, exp, grad, inner, sqrt)
    from fedm_amd.cases import streamer
    from fedm_amd.physical_constants import elementary_charge, epsilon_0
    from fedm_amd.termsum import parse
    forms.parameters["form_compiler"]["quadrature_degree"] = 2
    ME = FunctionSpace(mesh, MixedElement([FiniteElement()] * 3))
    u, v = TrialFunction(ME), TestFunctions(ME)
    E = -grad(u[2])
    E_m = sqrt(inner(-grad(u[2]), -grad(u[2])))
    mu = [wr.MU_ION, parse(streamer.MU_E)]
    D = [wr.D_ION, parse(streamer.D_E)]
    alpha = (1.1944e6 + 4.3666e26 * E_m ** (-3)) * exp(-2.73e7 / E_m) - 340.75
    f = [alpha * mu[1] * E_m * exp(u[1]), alpha * mu[1] * E_m * exp(u[1]), Function(FunctionSpace(mesh, FiniteElement()))]
    sign = [1.0, -1.0]
    for i in range(2):
        f[2] += sign[i] * exp(u[i]) * elementary_charge / epsilon_0
    dt = Expression("time_step", time_step=5e-12)
    r = Expression("x[0]", degree=1)
    eqt = ["drift-diffusion-reaction", "drift-diffusion-reaction"]
    Gamma = [ff.Flux(sign[i], u[i], D[i], mu[i], E, grad_diffusion=False) for i in range(2)]
    F = 0.0
    for i in range(2):
        F += ff.weak_form_balance_equation_log_representation(eqt[i], dt, dt, dx, u[i], None, None, v[i], f[i],
                                                              Gamma[i], r, D[i])
    F += ff.weak_form_Poisson_equation(dx, u[2], v[2], f[2], r)
    normal = FacetNormal(mesh)
    dsm = Measure("ds", domain=mesh, subdomain_data=ff.Marking_boundaries(mesh, streamer.BOUNDARIES))
    if ion_flux == "sum":
        ion = ff.Max(dot(Gamma[0], normal), 0.0)
    elif ion_flux == "electrons":
        ion = ff.Max(dot(Gamma[1], normal), 0.0) + ff.Max(dot(ff.Flux(1.0, u[0], D[0], mu[0], E), normal), 0.0)
    else:
        ion = ion_flux
    role, vth = ["Heavy", "electrons"], [wr.VTH_ION, vth_e]
    mu_wall = [mu[0], mu[1] if mu_wall_e is None else mu_wall_e]
    for i in range(2):
        F += ff.Boundary_flux("flux source", eqt[i], role[i], sign[i], mu_wall[i], E, normal, u[i], gamma, v[i], dsm(wr.CATHODE), r,
                              vth=vth[i], ref=0.3, Ion_flux=ion)
    F += ff.Boundary_flux("Neumann", eqt[1], role[1], sign[1], mu[1], E, normal, u[1], 0.0, v[1], dsm(wr.OUTER), r)
    return F


def test_facade_lowers_flux_source_walls():
    from fedm_amd import _lib, functions as ff
    from fedm_amd.mesh import RectangleMesh
    mesh = RectangleMesh((0, 0), (0.0125, 0.0125), 4, 4)
    m, mesh2, tags = ff.compile_forms(_wall_forms(mesh))
    md = m.to_c()
    wd = m.walls_to_c()
    assert md.n_tags == 4 and _lib.BC_KINDS["flux source"] == 2
    kinds = [[md.bc_kind[t][s] for s in range(2)] for t in range(4)]
    assert kinds == [[2, 2], [0, 0], [0, 0], [0, 1]]
    assert [wd.vth[0][s] for s in range(2)] == [wr.VTH_ION, wr.VTH_E]
    assert [wd.ref[0][s] for s in range(2)] == [0.3, 0.3]
    assert [wd.gamma[t] for t in range(4)] == [0.07, 0.0, 0.0, 0.0]
    assert [wd.emits[s] for s in range(4)] == [0, 1, 0, 0] and [wd.is_ion[s] for s in range(4)] == [1, 0, 0, 0]
    # Ion_flux = 0 goes with gamma = 0 only
    m0, _, _ = ff.compile_forms(_wall_forms(mesh, ion_flux=0.0, gamma=0.0))
    w0 = m0.walls_to_c()
    assert w0.gamma[0] == 0.0 and [w0.is_ion[s] for s in range(2)] == [0, 0] and w0.emits[1] == 1


def test_facade_refuses_what_the_kernels_do_not_evaluate():
    from fedm_amd import forms, functions as ff
    from fedm_amd.mesh import RectangleMesh
    mesh = RectangleMesh((0, 0), (0.0125, 0.0125), 4, 4)
    field = forms.Function(forms.FunctionSpace(mesh, forms.FiniteElement()))
    with pytest.raises(ValueError, match="species 1 on tag 1.*vth and ref must be numbers"):
        ff.compile_forms(_wall_forms(mesh, vth_e=field))
    with pytest.raises(ValueError, match="species 1 on tag 1.*mu and sign must be those of the species' Flux"):
        ff.compile_forms(_wall_forms(mesh, mu_wall_e=wr.MU_ION))
    with pytest.raises(ValueError, match="species 1 on tag 1.*Ion_flux must be"):
        ff.compile_forms(_wall_forms(mesh, ion_flux=3.0))
    with pytest.raises(ValueError, match="species 1 on tag 1.*Ion_flux must be"):
        ff.compile_forms(_wall_forms(mesh, ion_flux=0.0))                       # 0 with gamma = 0.07
    with pytest.raises(ValueError, match="species 1 on tag 1.*Flux of the ions' balance equations"):
        ff.compile_forms(_wall_forms(mesh, ion_flux="electrons"))


def test_models_without_walls_keep_their_descriptor_bytes():
    """fedm_model_desc does not move and a model without 'flux source' entries fills it as before: the benchmark
    model's descriptor has the size and the digest it had before walls existed (taken from Model.to_c() then)."""
    import ctypes as C
    import hashlib
    from fedm_amd import _lib
    from fedm_amd.cases import streamer
    from fedm_amd.device import Walls
    model = streamer.model()
    md = model.to_c()
    assert model.walls is None and model.walls_to_c() is None
    assert C.sizeof(_lib.ModelDesc) == 7232 and C.sizeof(_lib.WallDesc) == (2 * 8 * 4 + 8) * 8 + 2 * 4 * 4
    assert hashlib.sha256(bytes(md)).hexdigest() == "3a6e88c1d4a62fda7969e2f813843e4b566646217b71497c04503ecf27fc9bef"
    # a wall description that no entry of bc_kind refers to changes nothing and is not handed on
    again = streamer.model()
    again.walls = Walls(**wr.two_species_walls())
    assert bytes(again.to_c()) == bytes(md) and again.walls_to_c() is None
