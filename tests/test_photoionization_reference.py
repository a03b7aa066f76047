"""The photoionisation restatement (tests/photoionization_reference.py) pinned on something it did not write, and the
host side of the feature: the façade's lowering and every refusal that needs no GPU.

Manufactured solution: constant rate R on a strip, ``y = 0`` on the two ends ``z = 0, d``, zero flux on the sides:
``y(z) = (eta R / kappa^2) (1 - cosh(kappa (z - d/2)) / cosh(kappa d / 2))``, the same in the plane and in (r, z).
MEASURED (max nodal error, kappa d = 6, meshes of 4x8, 8x16, 16x32 cells): plane 1.23e-3, 3.15e-4, 7.95e-5 -- observed
orders 1.96 and 1.99; axisymmetric 1.61e-3, 4.16e-4, 1.05e-4 -- orders 1.95 and 1.98 (theory 2; the bound 1.8 leaves
the pre-asymptotic range its margin).  Largest spread of the axisymmetric solution over r at fixed z: 1.66e-3, 4.48e-4,
1.18e-4, against twice the plane error (two values that are each within e of y(z) differ by at most 2 e).
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import photoionization_reference as pr  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
D, LX, KAPPA, ETA, RATE = 1.0, 0.5, 6.0, 0.3, 7.0
SIZES = (8, 16, 32)


def _strip(n, axisymmetric):
    from oracle.forms import LFAModel
    from oracle.mesh import mark_boundaries, rectangle_right
    mesh = rectangle_right(0.0, 0.0, LX, D, n // 2, n)
    tags = mark_boundaries(mesh, [["line", 0.0, 0.0, 0.0, LX], ["line", D, D, 0.0, LX]])     # the two ends
    om = LFAModel(mesh, n_species=1, poisson=False, eq_type=["reaction"], Z=[0.0], facet_tags=tags,
                  bc_type=[["zero flux"], ["zero flux"]], qdeg=2, axisymmetric=axisymmetric)
    A, mask = pr.operators(om, [KAPPA], [1, 2])
    g = np.where(mask, 0.0, pr.load_vector(om, RATE, ETA))
    return mesh, pr.solve(A[0], g, mask), mask


@pytest.fixture(scope="module")
def strips():
    return {(n, axi): _strip(n, axi) for n in SIZES for axi in (False, True)}


def _errors(strips, axi):
    return [np.abs(strips[n, axi][1] - pr.exact_strip(strips[n, axi][0].coords[:, 1], D, KAPPA, ETA * RATE)).max()
            for n in SIZES]


def test_manufactured_solution_in_the_plane(strips):
    e = _errors(strips, False)
    orders = [np.log2(e[k] / e[k + 1]) for k in range(len(e) - 1)]
    print("plane: errors", e, "orders", orders)
    assert all(o >= 1.8 for o in orders)
    for n in SIZES:
        mesh, y, mask = strips[n, False]
        assert mask.sum() == 2 * (n // 2 + 1) and (y[mask] == 0.0).all()


def test_axisymmetric_solution_does_not_depend_on_r(strips):
    e_plane, e_axi = _errors(strips, False), _errors(strips, True)
    orders = [np.log2(e_axi[k] / e_axi[k + 1]) for k in range(len(e_axi) - 1)]
    print("axisymmetric: errors", e_axi, "orders", orders)
    assert all(o >= 1.8 for o in orders)
    for n, e in zip(SIZES, e_plane):
        mesh, y, _ = strips[n, True]
        z = mesh.coords[:, 1]
        spread = max(np.ptp(y[z == zz]) for zz in np.unique(z))
        print(n, "spread over r", spread, "plane error", e)
        assert spread <= 2.0 * e


def test_load_vector_and_table_restatements_agree_with_their_definitions():
    """sum_a g_a = int eta R w (the basis sums to one) and the table gathers sum_m c_m y_m by cell vertex."""
    from oracle import streamer as ost
    from oracle.mesh import rectangle_right
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, 5, 7)
    om = ost.build(mesh)
    U = pr.perturbed(ost.initial_state(om), 3)
    rate = pr.rate_at_points(om, U, [0])
    g = pr.load_vector(om, rate, 0.25)
    _, _, Em = om.cell_fields(U)
    total = 0.0
    from oracle.quadrature import triangle_rule
    xq, wq = triangle_rule(2)
    for q, (xi, w) in enumerate(zip(xq, wq)):
        phi = np.array([1.0 - xi[0] - xi[1], xi[0], xi[1]])
        n_e = np.exp(U[mesh.cells][:, :, 1] @ phi)
        total += (w * om.detJ * (om.xc[:, :, 0] @ phi) * 0.25 * om.reactions[0][0](Em)[0] * n_e).sum()
    # (the deck's alpha is the NET ionisation coefficient: negative, attachment, where the field is low)
    assert g.sum() == pytest.approx(total, rel=1e-13) and total != 0.0
    y = np.arange(2 * mesh.nv, dtype=float).reshape(2, mesh.nv)
    t = pr.table(om, y, [2.0, 0.5])
    assert t.shape == (mesh.nc, 3) and t[4, 2] == 2.0 * y[0, mesh.cells[4, 2]] + 0.5 * y[1, mesh.cells[4, 2]]


# ---- layers 3 and 4 without a GPU ------------------------------------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("streamer_example_photo", ROOT / "examples" / "streamer_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lowered(tmp_path, **kw):
    from fedm_amd import functions as ff
    mod, seen = _example(), {}

    class Stop(Exception):
        pass

    def capture(J, F, bcs):
        seen.update(F=F)
        raise Stop
    with pytest.raises(Stop):
        mod.main(cells=8, output_dir=tmp_path, quiet=True, stop_before_device=capture, **kw)
    return ff.compile_forms(seen["F"]), mod


def test_the_facade_lowers_the_source_to_the_model(tmp_path):
    from fedm_amd.cases import streamer
    (model, mesh, tags), mod = _lowered(tmp_path / "on", photoionization=True)
    ph = model.photoionization
    assert ph is not None and list(ph.reactions) == [0] and list(ph.targets) == [0, 1] and list(ph.zero_tags) == [1, 2]
    assert ph.efficiency == pytest.approx(0.075 * 30.0 / 780.0)
    assert list(ph.c) == pytest.approx([1e4 * a * 150.0 ** 2 for a in mod.PHOTO_A], rel=1e-15)
    assert list(ph.kappa) == pytest.approx([1e2 * v * 150.0 for v in mod.PHOTO_LAMBDA], rel=1e-15)
    assert ph.rtol == 1e-6 and ph.multigrid
    assert tags is not None and model.source_table_degrees() == [1, 1]
    md = model.to_c()
    assert list(md.ext_nodes)[:2] == [3, 3] and len(model.reactions) == 1
    same = streamer.default_photoionization()
    assert list(same.c) == pytest.approx(list(ph.c)) and list(same.kappa) == pytest.approx(list(ph.kappa))
    d = ph.to_c()
    assert (d.n_terms, d.n_src, d.target_species_mask, d.zero_tag_mask, d.src_reaction[0]) == (3, 1, 3, 3, 0)
    # off by default: the model of the benchmark's case 1, byte for byte
    (plain, _, _), _ = _lowered(tmp_path / "off")
    assert plain.photoionization is None and plain.source_table_degrees() == [0, 0]
    model.photoionization = None
    assert bytes(model.to_c()) == bytes(plain.to_c())


def _small_form(source_of, poisson_extra=None):
    """Two balances + Poisson on a small mesh; source_of(production, u, ds, fem) -> [f_ions, f_electrons]."""
    from fedm_amd import forms as fem, functions as ff
    from fedm_amd.physical_constants import elementary_charge, epsilon_0
    mesh = fem.RectangleMesh((0.0, 0.0), (1.0, 1.0), 3, 3)
    wall = ff.Marking_boundaries(mesh, [["line", 0.0, 0.0, 0.0, 1.0], ["line", 1.0, 1.0, 0.0, 1.0]])
    ds = fem.Measure("ds", domain=mesh, subdomain_data=wall)
    dx = fem.Measure("dx", domain=mesh)
    P1 = fem.FiniteElement("Lagrange", mesh.ufl_cell(), 1)
    W = fem.FunctionSpace(mesh, fem.MixedElement([P1, P1, P1]))
    u, v = fem.TrialFunction(W), fem.TestFunctions(W)
    old, old1 = fem.Function(W), fem.Function(W)
    E_m = fem.sqrt(fem.inner(-fem.grad(u[2]), -fem.grad(u[2])))
    mu = 2.0 * E_m ** (-0.25)
    production = 3.0 * mu * E_m * fem.exp(u[1])
    f = source_of(production, u, ds, fem)
    dt = fem.Expression("time_step", time_step=1e-12, degree=0)
    r = fem.Expression("x[0]", degree=1)
    flux = ff.Flux(-1.0, u[1], 0.1, mu, -fem.grad(u[2]), grad_diffusion=False)
    F = ff.weak_form_balance_equation_log_representation("reaction", dt, dt, dx, u[0], old[0], old1[0], v[0], f[0], 0.0, r)
    F += ff.weak_form_balance_equation_log_representation("drift-diffusion-reaction", dt, dt, dx, u[1], old[1], old1[1],
                                                          v[1], f[1], flux, r, 0.1)
    rho = (fem.exp(u[0]) - fem.exp(u[1])) * elementary_charge / epsilon_0
    if poisson_extra is not None:
        rho = rho + poisson_extra(production, ds)
    F += ff.weak_form_Poisson_equation(dx, u[2], v[2], rho, r)
    return F


def test_facade_lowering_and_refusals():
    from fedm_amd import forms as fem, functions as ff
    photo_args = dict(efficiency=0.1, A=[2.0, 3.0], lam=[0.5, 0.25], p_O2=10.0)

    def with_photo(production, u, ds, fem_):
        s = ff.Photoionization_source(production, zero_on=[ds(2)], **photo_args)
        return [production + s, s + production]
    model, mesh, tags = ff.compile_forms(with_photo_form := _small_form(with_photo), quadrature_degree=2)
    ph = model.photoionization
    assert list(ph.targets) == [0, 1] and list(ph.reactions) == [0] and list(ph.zero_tags) == [2]
    assert list(ph.c) == [1e4 * 2.0 * 100.0, 1e4 * 3.0 * 100.0] and list(ph.kappa) == [1e2 * 0.5 * 10.0, 1e2 * 0.25 * 10.0]
    assert tags is not None and len(model.bc_kind) == 2 and len(model.reactions) == 1
    assert with_photo_form is not None

    # the source alone on one species: only that species is a target
    def electrons_only(production, u, ds, fem_):
        return [production, production + ff.Photoionization_source(production, zero_on=[ds(1)], **photo_args)]
    assert list(ff.compile_forms(_small_form(electrons_only), quadrature_degree=2)[0].photoionization.targets) == [1]

    # an ionisation rate that is no reaction of the model's sources
    def foreign(production, u, ds, fem_):
        return [production, production + ff.Photoionization_source(5.0 * fem_.exp(u[0]), zero_on=[ds(1)], **photo_args)]
    with pytest.raises(ValueError, match="term 0 of the ionisation rate .* is not a reaction"):
        ff.compile_forms(_small_form(foreign), quadrature_degree=2)

    # the source on the right-hand side of the Poisson equation
    def plain(production, u, ds, fem_):
        return [production, production]
    with pytest.raises(ValueError, match="not to the right-hand side of the Poisson equation"):
        ff.compile_forms(_small_form(plain, lambda production, ds: ff.Photoionization_source(
            production, zero_on=[ds(1)], **photo_args)), quadrature_degree=2)

    # two different sources in one form
    def two(production, u, ds, fem_):
        return [production + ff.Photoionization_source(production, zero_on=[ds(1)], **photo_args),
                production + ff.Photoionization_source(production, zero_on=[ds(1)], **photo_args)]
    with pytest.raises(ValueError, match="two different photoionisation sources"):
        ff.compile_forms(_small_form(two), quadrature_degree=2)
    s1 = ff.Photoionization_source(3.0 * fem.exp(fem.Unknown(None, 1)), **photo_args)
    s2 = ff.Photoionization_source(3.0 * fem.exp(fem.Unknown(None, 1)), **photo_args)
    with pytest.raises(ValueError, match="two different photoionisation sources"):
        (1.0 * fem.exp(fem.Unknown(None, 1)) + s1) + s2
    # an Expression source and this term on one species
    with pytest.raises(ValueError, match="both an Expression source"):
        fem.Expression("x[0]", degree=1) + s1
    with pytest.raises(ValueError, match="both an Expression source"):
        s1 + fem.Expression("x[0]", degree=1)
    # the non-LFA family: nodal coefficients
    nodal = fem.Function(fem.FunctionSpace(fem.RectangleMesh((0.0, 0.0), (1.0, 1.0), 2, 2), "P", 1))
    nodal.vector()[:] = 2.0
    with pytest.raises(ValueError, match="LFA models only"):
        ff.Photoionization_source(nodal * fem.exp(fem.Unknown(None, 1)), **photo_args)
    with pytest.raises(ValueError, match="LFA models only"):
        (nodal + 1.0) * fem.exp(fem.Unknown(None, 1)) + s1
    # not a term that can be scaled or subtracted
    with pytest.raises(ValueError, match="can only be added"):
        2.0 * (1.0 * fem.exp(fem.Unknown(None, 1)) + s1)
    # arguments
    with pytest.raises(ValueError, match="one A per lam"):
        ff.Photoionization_source(3.0 * fem.exp(fem.Unknown(None, 1)), 0.1, [1.0], [1.0, 2.0], 10.0)
    with pytest.raises(ValueError, match="must be positive"):
        ff.Photoionization_source(3.0 * fem.exp(fem.Unknown(None, 1)), 0.1, [1.0], [-1.0], 10.0)
    with pytest.raises(ValueError, match=r"boundary measures ds\(tag\)"):
        ff.Photoionization_source(3.0 * fem.exp(fem.Unknown(None, 1)), 0.1, [1.0], [1.0], 10.0, zero_on=[fem.dx])


def test_model_level_refusals():
    """Layer 3 without a device: what DeviceProblem would hand to the library is checked when the descriptor is made."""
    import dataclasses
    from fedm_amd.cases import streamer
    from fedm_amd.device import Photoionization
    good = dict(reactions=[0], efficiency=0.1, c=[1.0, 2.0], kappa=[3.0, 4.0], targets=[0, 1], zero_tags=[1, 2])

    def refused(match, model=None, **change):
        m = model or streamer.model()
        m.photoionization = Photoionization(**{**good, **change})
        with pytest.raises(ValueError, match=match):
            m.to_c()
    refused("1 to 4 Helmholtz terms", c=[1.0] * 5, kappa=[1.0] * 5)
    refused("1 to 4 Helmholtz terms", c=[], kappa=[])
    refused("one c and one kappa", c=[1.0], kappa=[1.0, 2.0])
    refused("kappa must be positive", kappa=[3.0, 0.0])
    refused("kappa must be positive", kappa=[3.0, float("nan")])
    refused("reactions must index", reactions=[1])
    refused("reactions must index", reactions=[])
    refused("targets must be species", targets=[2])
    refused("zero_tags must be boundary tags", zero_tags=[5])
    refused("rtol must be positive", rtol=0.0)
    refused("Expression source of degree 2", model=dataclasses.replace(streamer.model(), ext_source_degree=[0, 2]))
    ok = streamer.model()
    ok.photoionization = Photoionization(**good)
    assert list(ok.to_c().ext_nodes)[:2] == [3, 3]
    one = streamer.model()
    one.photoionization = Photoionization(**{**good, "targets": [1]})
    assert list(one.to_c().ext_nodes)[:2] == [0, 3]


def test_host_operators_agree_with_the_restatement():
    """fedm_amd/photo.py (what DeviceProblem uploads) against tests/photoionization_reference.py, entry by entry."""
    from oracle import streamer as ost
    from oracle.mesh import rectangle_right
    from fedm_amd import photo
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Marking_boundaries, Mesh
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, 5, 7)
    om = ost.build(mesh)
    tags = Marking_boundaries(Mesh(mesh.coords, mesh.cells), streamer.BOUNDARIES)
    for axi in (True, False):
        om.axisymmetric = axi
        K, M = photo.helmholtz_matrices(mesh.coords, mesh.cells, axi, 2)
        Kr, Mr = pr.matrices(om)
        assert abs(K - Kr).max() <= 1e-14 * abs(Kr).max() and abs(M - Mr).max() <= 1e-14 * abs(Mr).max()
        fixed = photo.zero_vertices(mesh.cells, tags, [1, 2], mesh.nv)
        assert np.array_equal(fixed, pr.zero_mask(om, [1, 2])) and fixed.sum() == 12
        A = photo.eliminate(K + 9.0 * M, fixed)
        Ar = pr.eliminate(Kr + 9.0 * Mr, fixed)
        assert abs(A - Ar).max() <= 1e-14 * abs(Ar).max()
        assert (A.diagonal()[fixed] == 1.0).all() and abs(A - A.T).max() == 0.0
