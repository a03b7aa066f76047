"""The numpy restatement of the field output (tests/field_output_reference.py) and the host's point location
(fedm_amd/field_output.py) pinned on closed forms, on a 4 x 4 planar and an axisymmetric mesh.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import field_output_reference as fr  # noqa: E402

EPS = np.finfo(np.float64).eps


def _model(axisymmetric):
    from oracle import streamer as ost
    from oracle.mesh import rectangle_right
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, 4, 4)
    om = ost.build(mesh)
    if not axisymmetric:
        om.axisymmetric = False
        om._geometry()
    return om


@pytest.fixture(scope="module", params=[True, False], ids=["axisymmetric", "planar"])
def om(request):
    return _model(request.param)


def _linear_state(om, a=-3.1e5, b=1.7e6, ln_ni=33.0, ln_ne=35.5):
    r, z = om.mesh.coords[:, 0], om.mesh.coords[:, 1]
    return np.column_stack([np.full(om.mesh.nv, ln_ni), np.full(om.mesh.nv, ln_ne), a * r + b * z]), a, b


def test_a_linear_potential_gives_its_field_at_every_vertex_under_both_projections(om):
    U, a, b = _linear_state(om)
    for name, exact in (("E_r", -a), ("E_z", -b), ("E_norm", np.hypot(a, b))):
        p = fr.reference(om, U, name)
        for X in (fr.lumped(p), fr.consistent(om, p)):
            assert np.abs(X - exact).max() <= 1e-12 * abs(exact), name


def test_a_constant_density_gives_the_rate_k_n_to_the_p(om):
    U, a, b = _linear_state(om)
    k, P, _ = om.reactions[0]
    exact = k(np.array([np.hypot(a, b)]))[0][0] * np.exp(33.0) ** P[0] * np.exp(35.5) ** P[1]
    assert exact != 0.0                  # (negative at this field: the fit's attachment term outweighs ionisation)
    p = fr.reference(om, U, "rate:0")
    for X in (fr.lumped(p), fr.consistent(om, p)):
        assert np.abs(X - exact).max() <= 1e-12 * abs(exact)


def test_the_flux_of_a_uniform_density_is_its_drift(om):
    U, a, b = _linear_state(om)
    n_e, Em = np.exp(35.5), np.array([np.hypot(a, b)])
    mu = om.mu[1](Em)[0][0]
    for name, E in (("flux_r:1", -a), ("flux_z:1", -b)):
        exact = n_e * om.Z[1] * mu * E
        assert np.abs(fr.lumped(fr.reference(om, U, name)) - exact).max() <= 1e-12 * abs(exact)
    assert np.all(fr.lumped(fr.reference(om, U, "flux_z:0")) == 0.0)         # a 'reaction' species has no flux


def test_the_consistent_projection_of_a_p1_function_is_that_function(om):
    r, z = om.mesh.coords[:, 0], om.mesh.coords[:, 1]
    g = 2.0 + 3.0 * r / r.max() - 1.5 * z / z.max() + np.random.default_rng(5).normal(0, 0.3, om.mesh.nv)
    gc = g[om.mesh.cells]
    p = fr.load(om, [[gc @ phi] for phi, _ in fr.points(om)])                # (the degree-2 rule integrates P1 x P1)
    assert np.abs(fr.consistent(om, p) - g).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(fr.lumped(p) - g).max() > 1e-3                             # ... and the lumped one is not


def test_the_lumped_masses_add_up_to_the_area(om):
    from oracle import streamer as ost
    m = fr.lumped_mass(om)
    assert abs(m.sum() - ost.BOX ** 2) <= 8 * EPS * ost.BOX ** 2
    assert np.abs(np.asarray(fr.mass_matrix(om).sum(axis=1)).ravel() - m).max() <= 8 * EPS * m.max()
    from fedm_amd import field_output
    M = field_output.mass_matrix(om.mesh.coords, om.mesh.cells)
    assert abs(M - fr.mass_matrix(om)).max() <= 8 * EPS * m.max()


def test_pointwise_kinds(om):
    from oracle.forms import elementary_charge
    U, _, _ = _linear_state(om)
    assert np.array_equal(fr.reference(om, U, "state:2").value, U[:, 2])
    assert np.array_equal(fr.reference(om, U, "density:1").value, np.exp(U[:, 1]))
    c = fr.reference(om, U, "charge")
    exact = elementary_charge * (np.exp(33.0) - np.exp(35.5))
    assert np.abs(c.value - exact).max() <= 2 * EPS * abs(exact)
    assert np.all(c.abs >= np.abs(c.value))


# ---- point location ---------------------------------------------------------------------------------------------------
def _mesh():
    return _model(True).mesh


def _containing(mesh, p, tol=1e-12):
    """The cells that hold p, by an independent test: three signed areas."""
    x = mesh.coords[mesh.cells]
    out = []
    for c in range(mesh.nc):
        a, b, d = x[c]
        det = (b[0] - a[0]) * (d[1] - a[1]) - (b[1] - a[1]) * (d[0] - a[0])
        l = [((b[0] - p[0]) * (d[1] - p[1]) - (b[1] - p[1]) * (d[0] - p[0])) / det,
             ((d[0] - p[0]) * (a[1] - p[1]) - (d[1] - p[1]) * (a[0] - p[0])) / det,
             ((a[0] - p[0]) * (b[1] - p[1]) - (a[1] - p[1]) * (b[0] - p[0])) / det]
        if min(l) >= -tol:
            out.append(c)
    return out


def test_point_location_of_vertices_edge_midpoints_and_centroids():
    from fedm_amd import field_output
    mesh = _mesh()
    x = mesh.coords[mesh.cells]
    mids = np.concatenate([(x[:, i] + x[:, (i + 1) % 3]) / 2.0 for i in range(3)])
    cents = x.mean(axis=1)
    pts = np.concatenate([mesh.coords, mids, cents])
    cell, w = field_output.locate_points(mesh.coords, mesh.cells, pts)
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 2 * EPS
    for k, p in enumerate(pts):
        holders = _containing(mesh, p)
        assert cell[k] == holders[0], (k, cell[k], holders)                  # a tie goes to the lowest cell index
        assert np.abs(w[k] @ mesh.coords[mesh.cells[cell[k]]] - p).max() <= 4 * EPS * np.abs(mesh.coords).max()
    nv = mesh.nv
    assert all(len(_containing(mesh, p)) >= 2 for p in pts[:nv][[5, 6, 12]])        # interior vertices: really ties
    # a vertex gets the weights (1, 0, 0) in some order, a centroid three thirds
    assert np.all(np.sort(w[:nv], axis=1) == np.array([0.0, 0.0, 1.0]))
    assert np.abs(w[nv + mids.shape[0]:] - 1.0 / 3.0).max() <= 4 * EPS
    assert np.array_equal(cell[nv + mids.shape[0]:], np.arange(mesh.nc))


def test_a_point_outside_the_mesh_raises_and_is_named():
    from oracle import streamer as ost
    from fedm_amd import field_output
    mesh = _mesh()
    pts = np.array([[0.5 * ost.BOX, 0.5 * ost.BOX], [1.5 * ost.BOX, 0.25 * ost.BOX]])
    with pytest.raises(ValueError, match="point 1 .*outside"):
        field_output.locate_points(mesh.coords, mesh.cells, pts)
    with pytest.raises(ValueError, match="point 0 .*outside"):
        field_output.locate_points(mesh.coords, mesh.cells, [[-1e-6, 0.0]])


def test_chunks_do_not_change_the_answer():
    from fedm_amd import field_output
    mesh = _mesh()
    pts = np.random.default_rng(3).uniform(0.0, mesh.coords.max(), (37, 2))
    whole = field_output.locate_points(mesh.coords, mesh.cells, pts)
    parts = field_output.locate_points(mesh.coords, mesh.cells, pts, chunk=5 * mesh.nc)
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])


def test_output_times_are_the_times_file_output_writes():
    from fedm_amd import mesh_io

    class Recorder:
        mesh = object()

        def __init__(self):
            self.times = []

        def write(self, values, name, t):
            self.times.append(t)
    windows = [1e-11, 1e-10, 1e-9]
    rng = np.random.default_rng(11)
    t, t_out, step, t_out2, step2 = 0.0, windows[0], windows[0], windows[0], windows[0]
    new, old = [np.ones(3)], [np.zeros(3)]
    for _ in range(400):
        t_before, t = t, t + rng.uniform(1e-12, 4e-11)
        rec = Recorder()
        times, (t_out2, step2) = mesh_io.output_times(t, t_out2, step2, windows, windows)
        t_out, step = mesh_io.file_output(t, t_before, t_out, step, windows, windows, ["pvd"], [rec], ["x"], new, old)
        assert times == rec.times and (t_out2, step2) == (t_out, step)
    assert t > windows[-1]                                    # all three windows and the stretch past the last one


def test_field_names():
    from fedm_amd import field_output as fo
    assert fo.parse_request("E_norm", 2, 3, 1) == (5, 0)
    assert fo.parse_request("density:electrons", 2, 3, 1, ("ions", "electrons")) == (1, 1)
    assert fo.parse_request("flux_z:1", 2, 3, 1) == (8, 1)
    assert fo.parse_request(("rate", 0), 2, 3, 1) == (6, 0)
    for bad in ("density", "density:2", "rate:1", "speed", "charge:1", "density:neutrals"):
        with pytest.raises(ValueError):
            fo.parse_request(bad, 2, 3, 1, ("ions", "electrons"))
