"""tests/rank_assembly_reference.py and the inputs of the rank-assembly tests, checked on the CPU: the expected local
systems glue back to the global one, and the partitions put on the ranks what the GPU tests rely on (split electrodes,
wall cells across the cut, Dirichlet dofs on identity vertices)."""
import numpy as np
import pytest
import scipy.sparse as sp

import rank_assembly_reference as rr

NEQ = 3


@pytest.fixture(scope="module")
def case():
    return rr.wall_case(rr.mesh())


@pytest.fixture(scope="module")
def parts(case):
    msh = case["mesh"]
    return rr.partitions(msh.coords, msh.cells)


def _facets(msh, lm, tag):
    return int((rr.local_facet_tags(msh, lm) == tag).sum())


def _dirichlet_on_identity(lm):
    dofs, _ = rr.local_dirichlet(lm, NEQ)
    return int(np.isin(dofs // NEQ, rr.identity_vertices(lm)).sum())


def test_preconditions_of_the_global_state(case):
    """20 x 20: 40 wall facets, both signs of E.n on both electrodes, nothing near a kink (wall_flux_reference)."""
    info = case["info"]
    assert info["tags"] == [1, 2] and info["n_facets"] == 40
    assert info["min_En_over_E"] == pytest.approx(0.0133, abs=1e-4)


def test_the_partitions_are_the_explicit_ones(case, parts):
    msh = case["mesh"]
    r, z = msh.coords[:, 0], msh.coords[:, 1]
    assert sorted(parts) == ["r-cut", "three", "z-cut"]
    assert np.bincount(parts["r-cut"]).tolist() == [231, 210] and np.bincount(parts["z-cut"]).tolist() == [231, 210]
    assert np.bincount(parts["three"]).tolist() == [147, 147, 147]
    assert r[parts["r-cut"] == 0].max() < r[parts["r-cut"] == 1].min()
    assert z[parts["z-cut"] == 0].max() < z[parts["z-cut"] == 1].min()


@pytest.mark.parametrize("name", ["r-cut", "z-cut", "three"])
@pytest.mark.parametrize("depth", rr.DEPTHS)
def test_owned_rows_glue_back_to_the_global_system(case, parts, name, depth):
    msh, F, J = case["mesh"], case["F"], case["J"]
    N = F.size
    F_glued, blocks, seen = np.full(N, np.nan), [], np.zeros(N, dtype=int)
    for lm in rr.local_meshes(msh.coords, msh.cells, parts[name], depth):
        F_loc, J_loc, assembled = rr.expected_local_system(lm, F, J, NEQ)
        nloc = lm.coords.shape[0]
        assert F_loc.shape == (nloc * NEQ,) and J_loc.shape == (nloc * NEQ,) * 2
        # the assembled rows: layers below the depth; every other row is F = 0 and a unit row
        assert np.array_equal(assembled, np.repeat(lm.layer < lm.depth, NEQ))
        assert assembled[:lm.n_owned * NEQ].all()
        ident = np.nonzero(~assembled)[0]
        assert ident.size == NEQ * rr.identity_vertices(lm).size > 0
        if depth > 1:
            assert np.array_equal(rr.identity_vertices(lm), lm.identity_vertices)
        else:
            assert np.array_equal(rr.identity_vertices(lm), np.arange(lm.n_owned, nloc))
        assert np.all(F_loc[ident] == 0.0)
        Ji = J_loc[ident]
        assert Ji.nnz == ident.size and np.array_equal(Ji.indices, ident) and np.all(Ji.data == 1.0)
        # owned rows back into the global numbering
        gdof = (lm.vertex_global[:, None] * NEQ + np.arange(NEQ)[None, :]).ravel()
        own = np.arange(lm.n_owned * NEQ)
        F_glued[gdof[own]] = F_loc[own]
        seen[gdof[own]] += 1
        blk = J_loc[own].tocoo()
        blocks.append(sp.coo_matrix((blk.data, (gdof[own][blk.row], gdof[blk.col])), shape=(N, N)))
        # ... and the redundantly assembled ghost rows are the global rows as well
        red = np.nonzero(assembled)[0][lm.n_owned * NEQ:]
        assert np.array_equal(F_loc[red], F[gdof[red]])
    assert np.all(seen == 1)
    assert np.array_equal(F_glued, F)
    J_glued = sp.csr_matrix(sum(blocks))
    assert abs(J_glued - J).max() == 0.0
    assert J_glued.nnz == sp.csr_matrix(J).nnz


@pytest.mark.parametrize("depth", rr.DEPTHS)
def test_r_cut_splits_both_electrodes(case, parts, depth):
    """Every rank has facets of both electrodes, two wall cells that hold an owned and a ghost vertex, and two
    Dirichlet dofs on identity vertices (the double writer's input) at every depth."""
    msh = case["mesh"]
    expected = {1: [(11, 11), (10, 10)], 3: [(13, 13), (12, 12)], 8: [(18, 18), (17, 17)]}[depth]
    for lm, counts in zip(rr.local_meshes(msh.coords, msh.cells, parts["r-cut"], depth), expected):
        assert (_facets(msh, lm, 1), _facets(msh, lm, 2)) == counts
        tags = rr.local_facet_tags(msh, lm)
        wall = ((tags == 1) | (tags == 2)).any(axis=1)
        owned = lm.cells < lm.n_owned
        assert int((wall & owned.any(axis=1) & (~owned).any(axis=1)).sum()) == 2
        assert _dirichlet_on_identity(lm) == 2
        # ... where the wall state is off the electrode's value: F = 0 and F = u - value differ
        dofs, vals = rr.local_dirichlet(lm, NEQ)
        on_id = np.isin(dofs // NEQ, rr.identity_vertices(lm))
        u = rr.restrict(lm, case["states"][0]).ravel()
        assert np.abs(u[dofs[on_id]] - vals[on_id]).min() > 1.0


@pytest.mark.parametrize("depth", rr.DEPTHS)
def test_z_cut_gives_each_rank_one_electrode(case, parts, depth):
    msh = case["mesh"]
    for lm in rr.local_meshes(msh.coords, msh.cells, parts["z-cut"], depth):
        mine, other = (1, 2) if lm.rank == 0 else (2, 1)
        assert _facets(msh, lm, mine) == 20 and _facets(msh, lm, other) == 0
        assert _facets(msh, lm, 3) > 0 and _facets(msh, lm, 4) > 0        # the cut crosses the axis and r = BOX
        assert _dirichlet_on_identity(lm) == 0


@pytest.mark.parametrize("depth", rr.DEPTHS)
def test_three_parts_form_a_t_junction(case, parts, depth):
    msh = case["mesh"]
    lms = rr.local_meshes(msh.coords, msh.cells, parts["three"], depth)
    assert _facets(msh, lms[0], 1) > 0 and _facets(msh, lms[0], 2) > 0
    assert _facets(msh, lms[1], 1) > 0 and _facets(msh, lms[1], 2) == 0
    assert _facets(msh, lms[2], 1) == 0 and _facets(msh, lms[2], 2) > 0
    assert [len(lm.neighbours) for lm in lms] == [2, 2, 2]


def test_the_other_models_leave_the_dirichlet_values_too():
    """The streamer and the tabulated case: a state whose potential is off the electrodes' values, so that F of a
    Dirichlet row tells 0 from u - value."""
    msh = rr.mesh()
    for name in ("streamer", "tabulated"):
        c = rr.CASES[name](msh)
        om, U = c["om"], c["states"][0]
        assert np.abs(U.ravel()[om.dirichlet_dofs] - om.dirichlet_vals).min() > 1.0
        assert np.isfinite(c["F"]).all() and np.isfinite(c["J"].data).all()
