"""tests/diagnostics_reference.py pinned on closed forms (CPU), and the host-side checks of the diagnostics.

The box is axisymmetric, R x H = 2 mm x 5 mm, 5 x 7 cells (not square, h_r != h_z).  The integrands of the closed
forms are polynomials of degree <= 2 in (r, z) -- a constant density times the weight r, a constant field -- which the
degree-2 rule integrates exactly, so every check is held to 1e-13 relative.
"""
import math
import types

import numpy as np
import pytest

import diagnostics_reference as dref
import rank_assembly_reference as rr

R, H, V, N0 = 2.0e-3, 5.0e-3, 7.5e3, 3.0e15
TOL = 1e-13


def _close(a, b, scale=None):
    return abs(a - b) <= TOL * (abs(b) if scale is None else scale)


@pytest.fixture(scope="module")
def box():
    """The oracle's streamer model on the R x H box at uniform densities n_i = n_e = N0 and Phi = V z / H."""
    from oracle import streamer as ost
    from oracle.mesh import rectangle_right
    mesh = rectangle_right(0.0, 0.0, R, H, 5, 7)
    om = ost.build(mesh)
    z = mesh.coords[:, 1]
    U = np.column_stack([np.full(mesh.nv, math.log(N0)), np.full(mesh.nv, math.log(N0)), V * z / H])
    group = np.where(np.abs(z) < 1e-15, 1, np.where(np.abs(z - H) < 1e-15, 2, 0)).astype(np.int8)
    return types.SimpleNamespace(mesh=mesh, om=om, U=U, group=group, psi=z / H)


def test_uniform_density_integrates_to_the_volume(box):
    ref = dref.reference(box.om, box.U)
    for s in range(2):
        assert _close(ref["species"][s].value, N0 * math.pi * R ** 2 * H)
        assert _close(ref["species"][s].abs, N0 * math.pi * R ** 2 * H)      # every term is positive
    # planar: per metre of depth, w = 1 / (2 pi)
    from oracle import streamer as ost
    plane = ost.build(box.mesh)
    plane.axisymmetric = False
    plane._geometry()
    assert _close(dref.reference(plane, box.U)["species"][1].value, N0 * R * H)


def test_uniform_field_and_the_electrode_charges(box):
    ref = dref.reference(box.om, box.U, group=box.group, n_groups=2)
    Em = box.om.cell_fields(box.U)[2]
    assert np.abs(Em - V / H).max() <= TOL * V / H
    assert _close(ref["field"].value, V / H) and 0 <= ref["field"].index < box.mesh.nc
    q = math.pi * R ** 2 * V / H
    bottom, top = ref["groups"]
    assert _close(top.value, q) and _close(bottom.value, -q)
    # n_i = n_e: the charge terms cancel pairwise; what is left of the two sums cancels to rounding
    assert abs(top.value + bottom.value) <= TOL * q
    assert top.abs > q and bottom.abs > q      # ... while the charge terms are in sum |terms|


def test_induced_current_of_a_uniform_drift(box):
    ref = dref.reference(box.om, box.U, psi=box.psi)
    E = V / H
    mu_e = 2.3987 * E ** -0.26                                  # the deck's closed form (oracle.streamer.MU_E)
    expected = (-1.0) ** 2 * mu_e * E * N0 * math.pi * R ** 2
    assert _close(ref["current"].value, expected)
    # the diffusive part alone (no mobility): grad(u) = 0
    from oracle import streamer as ost
    from oracle.forms import TermSum
    nomu = ost.build(box.mesh)
    nomu.mu[1] = TermSum.const(0.0)
    assert abs(dref.reference(nomu, box.U, psi=box.psi)["current"].value) <= TOL * expected
    # no psi: no current
    assert dref.reference(box.om, box.U)["current"] == dref.Sum(0.0, 0.0)


def test_window_and_ties(box):
    """A uniform field is one big tie up to rounding; raise Phi at one vertex and the maximum is unique and found."""
    U = box.U.copy()
    v = int(np.argmin(np.abs(box.mesh.coords[:, 0] - 0.4e-3) + np.abs(box.mesh.coords[:, 1] - H * 3 / 7)))
    U[v, 2] += 0.5 * V
    ref = dref.reference(box.om, U, window=(0.0, R, 0.0, H))
    assert ref["field"].unique and v in box.mesh.cells[ref["field"].index]
    assert ref["window"] == ref["field"]
    empty = dref.reference(box.om, U, window=(2 * R, 3 * R, 0.0, H))["window"]
    assert empty.value == 0.0 and empty.index == -1
    cen = dref.centroids(box.om)[ref["field"].index]
    assert ref["field"].centroid == (cen[0], cen[1])
    nod = dref.reference(box.om, U)["nodal"]
    assert nod[0].index == 0 and not nod[0].unique and nod[0].value == math.log(N0)


@pytest.fixture(scope="module")
def rank_case():
    c = rr.streamer_case(rr.mesh())
    msh, om, U = c["mesh"], c["om"], c["states"][0]
    z = msh.coords[:, 1]
    from oracle import streamer as ost
    group = np.where(np.abs(z) < 3e-16, 1, np.where(np.abs(z - ost.BOX) < 3e-16, 2, 0)).astype(np.int8)
    psi = z / ost.BOX
    window = (0.0, 1.5e-3, 0.0, ost.BOX)
    glob = dref.reference(om, U, window=window, psi=psi, group=group, n_groups=2)
    return types.SimpleNamespace(mesh=msh, om=om, U=U, group=group, psi=psi, window=window, glob=glob,
                                 parts=rr.partitions(msh.coords, msh.cells))


@pytest.mark.parametrize("name", ["r-cut", "z-cut", "three"])
@pytest.mark.parametrize("depth", [1, 8])
def test_rank_shares_add_up(rank_case, name, depth):
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    c = rank_case
    shares, lms = [], rr.local_meshes(c.mesh.coords, c.mesh.cells, c.parts[name], depth)
    for lm in lms:
        lom = ost.build(OMesh(lm.coords, lm.cells))
        owned = np.arange(lm.coords.shape[0]) < lm.n_owned
        shares.append(dref.reference(lom, rr.restrict(lm, c.U), window=c.window, psi=rr.restrict(lm, c.psi),
                                     group=rr.restrict(lm, c.group), n_groups=2, owned=owned))

    def adds_up(pick):
        tot, g = dref.combine_sums([pick(s) for s in shares]), pick(c.glob)
        assert abs(tot.value - g.value) <= TOL * g.abs
    for s in range(2):
        adds_up(lambda r, s=s: r["species"][s])
        adds_up(lambda r, s=s: r["groups"][s])
    adds_up(lambda r: r["current"])
    assert c.glob["current"].value != 0.0 and c.glob["groups"][0].value != 0.0
    for key, to_global in (("field", [lm.cell_global for lm in lms]), ("window", [lm.cell_global for lm in lms])):
        assert c.glob[key].unique
        assert dref.combine_maxima([s[key] for s in shares], to_global) == (c.glob[key].value, c.glob[key].index)
    for s in range(2):
        got = dref.combine_maxima([r["nodal"][s] for r in shares], [lm.vertex_global for lm in lms])
        assert got == (c.glob["nodal"][s].value, c.glob["nodal"][s].index)
    if name == "r-cut":       # both electrodes are split: every rank holds a share of both group sums
        assert all(r["groups"][g].abs > 0.0 for r in shares for g in range(2))


# ---- host checks that need no GPU -------------------------------------------------------------------------------------
def test_the_entry_points_are_bound_under_abi_10():
    from fedm_amd import _lib
    assert _lib.ABI_VERSION == 10
    assert {"fedm_diag_setup", "fedm_diagnostics"} <= set(_lib.exported_symbols())
    # the structs as include/fedm_hip.h lays them out: 8-byte fields first, no padding inside
    import ctypes as C
    assert C.sizeof(_lib.DiagOpts) == 40 and C.sizeof(_lib.DiagOut) == 8 * (4 + 8 + 1 + 3 + 3 + 4) + 4 * (2 + 4 + 2)
    header = (rr.__file__ and __import__("pathlib").Path(rr.__file__).resolve().parents[1] / "include" / "fedm_hip.h")
    text = header.read_text()
    assert "#define FEDM_ABI_VERSION 10" in text and "fedm_diag_setup" in text and "fedm_diagnostics" in text


def _stub_device():
    """What Discharge_diagnostics reads before it touches the device: the streamer's 2 x 2 mesh with its tags."""
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Marking_boundaries, Mesh
    m = streamer.mesh(2)
    msh = Mesh(m.coords, m.cells)
    dofs, _ = streamer.dirichlet(msh.coords)
    return types.SimpleNamespace(model=streamer.model(), cells=msh.cells, coords=msh.coords, nv=msh.coords.shape[0],
                                 _tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                                 dirichlet_vertices=lambda: np.unique(dofs // 3))


def test_a_vertex_in_two_groups_is_refused():
    from fedm_amd import functions as ff
    from fedm_amd.device import boundary_vertex_groups
    dev = _stub_device()
    # tags 1, 2: the electrodes (Dirichlet); tag 3: the axis, whose two end vertices are electrode vertices
    with pytest.raises(ValueError, match="belongs to one group"):
        ff.Discharge_diagnostics(types.SimpleNamespace(device=dev), boundary_tags=(1, 3))
    g = boundary_vertex_groups(dev.cells, dev._tags, dev.nv, dev.dirichlet_vertices(), (1, 2))
    z = dev.coords[:, 1]
    assert np.array_equal(g, np.where(z == 0.0, 1, np.where(z == z.max(), 2, 0)))
    # only Dirichlet vertices are taken: the wall r = BOX alone gives its two corners
    g4 = boundary_vertex_groups(dev.cells, dev._tags, dev.nv, dev.dirichlet_vertices(), (4,))
    assert g4.sum() == 2


def test_an_lmea_model_is_refused():
    from fedm_amd import functions as ff
    from fedm_amd.device import GdModel
    dev = _stub_device()
    dev.model = object.__new__(GdModel)
    with pytest.raises(ValueError, match="LFA models only"):
        ff.Discharge_diagnostics(dev)
