"""What one rank of a partitioned mesh must hold after an assembly, from the global restatement (helper module, numpy).

A rank assembles the rows of its owned vertices and of its ghost vertices of the layers 1 .. depth-1
(fedm_amd/partition.py); every other local vertex -- all ghosts of a one-layer halo, the outermost layer of a deep one
-- has F = 0 and a unit row, whatever a Dirichlet value says about it.  ``expected_local_system`` cuts exactly that
out of the global F and J; ``partitions`` are the explicit vertex partitions the rank tests run on, and the ``*_case``
functions the three models with their global states, F and J (computed once by the caller, never changed).
"""
import numpy as np
import scipy.sparse as sp

DEPTHS = (1, 3, 8)
DT = (5e-12, 4e-12)


def mesh():
    """The 20 x 20 mesh of test_gpu_wall_flux.py's tensor_case."""
    from fedm_amd.cases import streamer
    return streamer.mesh(20, 2.0)


def partitions(coords, cells):
    """Named vertex partitions (part[v] = rank).  Explicit: the cut direction is not left to partition_rcb.
    'r-cut': both electrodes split between two ranks; 'z-cut': one electrode per rank, the cut crosses the Neumann
    wall r = BOX and the axis; 'three': a T-junction."""
    from fedm_amd import partition
    coords = np.asarray(coords)
    r, z = coords[:, 0], coords[:, 1]
    return {"r-cut": (r > np.median(r)).astype(np.int32),
            "z-cut": (z > np.median(z)).astype(np.int32),
            "three": partition.partition_rcb(coords, 3, cells)}


def local_meshes(coords, cells, part, depth):
    from fedm_amd import partition
    return [partition.local_mesh(coords, cells, part, rank, depth=depth) for rank in range(int(part.max()) + 1)]


def identity_vertices(lm):
    """Local ids of the vertices with identity rows: every local vertex whose layer is not below the depth."""
    return np.nonzero(lm.layer >= lm.depth)[0]


def expected_local_system(lm, F, J, neq):
    """(F_local, J_local as CSR, assembled) in ``lm``'s local numbering: the global rows, columns mapped through
    vertex_global, for the local vertices with layer < depth; F = 0 and a unit row for every other local vertex.
    ``assembled`` is the boolean mask of the assembled rows (per dof)."""
    g = np.asarray(lm.vertex_global, dtype=np.int64)
    nloc, N = g.size, np.asarray(F).size
    dof = np.arange(neq)
    gdof = (g[:, None] * neq + dof[None, :]).ravel()
    local_of_global = np.full(N, -1, dtype=np.int64)
    local_of_global[gdof] = np.arange(nloc * neq)
    assembled = np.repeat(lm.layer < lm.depth, neq)
    F_loc = np.where(assembled, np.asarray(F).ravel()[gdof], 0.0)
    rows = sp.csr_matrix(J)[gdof].tocoo()
    keep = assembled[rows.row]
    cols = local_of_global[rows.col[keep]]
    assert (cols >= 0).all(), "an assembled row reaches outside the local mesh"
    ident = np.nonzero(~assembled)[0]
    J_loc = sp.csr_matrix((np.concatenate([rows.data[keep], np.ones(ident.size)]),
                           (np.concatenate([rows.row[keep], ident]), np.concatenate([cols, ident]))),
                          shape=(nloc * neq, nloc * neq))
    return F_loc, J_loc, assembled


def restrict(lm, U):
    """A global nodal array (n_vertices, ...) on the local vertices."""
    return np.ascontiguousarray(np.asarray(U)[lm.vertex_global])


def local_facet_tags(msh, lm):
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Marking_boundaries
    return Marking_boundaries(msh, streamer.BOUNDARIES)[lm.cell_global]


def local_dirichlet(lm, neq):
    """The Dirichlet dofs of every local vertex (as streamer_distributed.Runner passes them), in the model's n_eq."""
    from fedm_amd.cases import streamer
    dofs, vals = streamer.dirichlet(lm.coords)
    return ((dofs // 3) * neq + neq - 1).astype(np.int32), vals


# ---- the models, their global states and the restatement's F and J ---------------------------------------------------
def _old_states(U):
    rng = np.random.default_rng(3)
    return U - 0.01 * rng.random(U.shape), U - 0.02 * rng.random(U.shape)


def wall_case(msh):
    """wall_flux_reference's two-species wall model at wall_state, which does not satisfy the Dirichlet values."""
    import wall_flux_reference as wr
    from oracle.mesh import Mesh as OMesh
    om = wr.set_dirichlet(wr.oracle_two_species(OMesh(msh.coords, msh.cells)), msh.coords)
    U = wr.wall_state(msh.coords)
    info = wr.assert_preconditions(om, U)
    assert np.abs(U.ravel()[om.dirichlet_dofs] - om.dirichlet_vals).max() > 1.0
    Uo, Uo1 = _old_states(U)
    F, J = om.residual_jacobian(U, Uo, Uo1, *DT)
    return dict(mesh=msh, om=om, model=wr.device_two_species_model, states=(U, Uo, Uo1), F=F, J=sp.csr_matrix(J),
                info=info)


def _perturbed_streamer_state(om):
    """The streamer's initial state (with its Poisson solve) plus smooth perturbations; the potential leaves the
    Dirichlet values as well."""
    from oracle import streamer as ost
    U = ost.initial_state(om)
    x, y = om.mesh.coords[:, 0] / ost.BOX, om.mesh.coords[:, 1] / ost.BOX
    U[:, 0] += 0.05 * np.sin(7.0 * x) * np.cos(5.0 * y)
    U[:, 1] += 0.3 * np.cos(3.0 * x) * np.sin(4.0 * y)
    U[:, 2] += 20.0 * (1.5 + np.cos(5.0 * x + 2.0 * y))
    return U


def streamer_case(msh):
    """The closed-form streamer (oracle.streamer.build against cases.streamer.model)."""
    from fedm_amd.cases import streamer
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    om = ost.build(OMesh(msh.coords, msh.cells))
    U = _perturbed_streamer_state(om)
    Uo, Uo1 = _old_states(U)
    F, J = om.residual_jacobian(U, Uo, Uo1, *DT)
    return dict(mesh=msh, om=om, model=streamer.model, states=(U, Uo, Uo1), F=F, J=sp.csr_matrix(J))


def tabulated_case(msh):
    """The tabulated streamer of tabulated_reference, knots from the quantiles of the global |E|."""
    import tabulated_reference as tr
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    omesh = OMesh(msh.coords, msh.cells)
    closed = ost.build(omesh)
    U = _perturbed_streamer_state(closed)
    x = tr.quantile_knots(closed.cell_fields(U)[2])
    om = tr.oracle_streamer(omesh, x)
    tr.assert_knots_exercise_the_lookup(x, om.cell_fields(U)[2])
    Uo, Uo1 = _old_states(U)
    F, J = om.residual_jacobian(U, Uo, Uo1, *DT)
    return dict(mesh=msh, om=om, model=lambda: tr.device_streamer_model(x), states=(U, Uo, Uo1), F=F,
                J=sp.csr_matrix(J), knots=x)


CASES = {"streamer": streamer_case, "tabulated": tabulated_case, "walls": wall_case}
