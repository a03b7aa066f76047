"""The numpy restatement of the LMEA coefficient refresh (tests/lmea_refresh_reference.py) against the oracle's own
statements of the same formulas (oracle/gd.py: ``reduced_field``, ``coefficients``), CPU only -- so that the GPU
tests of tests/test_gpu_lmea_refresh.py compare the device with something that has itself been compared.

Also measured here: how far Jacobi-CG at the device's tolerance (1e-14, at most 500 iterations) sits from the sparse
LU solve of the same mass system, as an algorithm in float64 numpy.  On the crossed 3x3, 1x21, 2x25, 10x10, 64x64,
128x128 meshes and the refined Delaunay mesh, with both potentials: 14..29 iterations, 3e-16..2.1e-14 of max |redE|.
The GPU tests bound the device's distance from LU by 1e-12 on that ground."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lmea_refresh_reference as ref  # noqa: E402

MESHES = {"crossed 10x10": lambda: ref.crossed(10, 10), "crossed 64x64": lambda: ref.crossed(64, 64),
          "refined": ref.refined}


@pytest.fixture(scope="module")
def deck():
    d = ref.read_deck()
    return d, ref.deck_programs(d)


@pytest.fixture(scope="module", params=list(MESHES))
def setup(request):
    from oracle import gd as ogd
    from oracle.mesh import Mesh as OMesh
    m = MESHES[request.param]()
    return m, ogd.GlowDischarge(ref.DECK / "4_particles", mesh=OMesh(m.coords, m.cells))


@pytest.mark.parametrize("which", ["ramp", "steep"])
def test_reduced_field_equals_the_oracles(setup, which):
    m, o = setup
    Phi = ref.potential(m.coords, which)
    mine = ref.reduced_field(m.coords, m.cells, o.N0, Phi)
    theirs = o.reduced_field(Phi)
    assert np.abs(theirs).max() > 100.0
    assert np.abs(mine - theirs).max() <= 1e-13 * np.abs(theirs).max()       # two LU solves of one system


@pytest.mark.parametrize("which", ["ramp", "steep"])
def test_jacobi_cg_reaches_lu_well_inside_its_iteration_limit(setup, which):
    m, o = setup
    M = ref.mass_matrix(m.coords, m.cells)
    b = ref.reduced_field_rhs(m.coords, m.cells, o.N0, ref.potential(m.coords, which))
    lu = ref.reduced_field(m.coords, m.cells, o.N0, ref.potential(m.coords, which), M)
    x, its = ref.jacobi_cg(M, b, 1e-14, 500)
    d = np.abs(x - lu).max() / np.abs(lu).max()
    print(f"{m.coords.shape[0]} vertices, {which}: {its} iterations, {d:.1e} from LU")
    assert its < 100
    assert d <= 1e-13


def test_deck_programs_give_the_oracles_coefficients(setup, deck):
    m, o = setup
    d, (tables, programs) = deck
    nv, ns, nr = m.coords.shape[0], d.ns, d.nr
    assert len(programs) == 4 * ns + 2 * nr + 3
    rng = np.random.default_rng(1)
    # energies past both ends of the electron tables, potential past the first knot of the E/N table
    me = np.exp(rng.uniform(np.log(1e-3), np.log(1e5), nv))
    U = rng.normal(0.0, 1.0, (nv, d.n_eq))
    U[:, -1] = ref.potential(m.coords, "steep")
    U_old = rng.normal(0.0, 1.0, (nv, d.n_eq))
    fields = rng.uniform(0.5, 2.0, (len(programs), nv))
    fields[-2] = me
    new, redE = ref.refresh(m.coords, m.cells, d.N0, tables, programs, fields, U, U_old)
    assert np.abs(redE - o.reduced_field(U[:, -1])).max() <= 1e-13 * np.abs(redE).max()
    assert (redE < 0).any() and me.min() < tables[1][0][0] and me.max() > tables[1][0][-1]
    co = o.coefficients(me, redE)
    rows = dict(mu=new[0:ns], D=new[ns:2 * ns], k=new[4 * ns:4 * ns + nr], kd=new[4 * ns + nr:4 * ns + 2 * nr])
    kinds = [p["kind"] for p in programs]
    checked = 0
    for name, block in rows.items():
        first = dict(mu=0, D=ns, k=4 * ns, kd=4 * ns + nr)[name]
        for i, row in enumerate(block):
            if kinds[first + i] == "keep":                       # 'const': set once, not the refresh's business
                assert np.array_equal(row, fields[first + i])
                continue
            assert np.allclose(row, co[name][i], rtol=1e-14, atol=0.0), (name, i)
            checked += 1
    assert np.allclose(new[2 * ns + ns - 1], co["mu_e_diff"], rtol=1e-14, atol=0.0)
    assert np.allclose(new[3 * ns + ns - 1], co["D_e_diff"], rtol=1e-14, atol=0.0)
    assert checked == kinds.count("table") + kinds.count("scaled_row") - 2
    # bookkeeping rows
    assert np.array_equal(new[-3], me) and np.array_equal(new[-2], me) and np.array_equal(new[-1], U_old[:, d.n_eq - 2])


def test_mean_energy_and_the_order_of_the_copy():
    U = np.array([[3.0, 0.0, 0.0, 1.0, 5.0], [40.0, 0.0, 0.0, 2.5, 5.0]])
    assert np.array_equal(ref.mean_energy(U), np.exp(np.array([2.0, 37.5])))
    # a one-row table evaluated at the energy: the OLD mean energy is the me row as it stood BEFORE the refresh
    coords = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    cells = np.array([[0, 1, 2]])
    progs = [dict(kind="table", table=0, arg="energy", scale=2.0), dict(kind="scaled_row", src_row=0, scale=3.0),
             dict(kind="me_old"), dict(kind="me"), dict(kind="ue_old")]
    fields = np.array([[9.0] * 3, [9.0] * 3, [1.0, 1.0, 1.0], [2.0, 3.0, 10.0], [0.0] * 3])
    new, redE = ref.refresh(coords, cells, 1e21, [(np.array([2.0, 4.0]), np.array([10.0, 30.0]))], progs, fields,
                            np.zeros((3, 3)), np.arange(9.0).reshape(3, 3))
    assert np.array_equal(redE, np.zeros(3))
    assert np.array_equal(new, [[20.0, 40.0, 60.0], [60.0, 120.0, 180.0], [2.0, 3.0, 10.0], [2.0, 3.0, 10.0],
                                [1.0, 4.0, 7.0]])
