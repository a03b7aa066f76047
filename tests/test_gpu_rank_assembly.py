"""The system ONE RANK assembles, row by row against the global restatement (tests/rank_assembly_reference.py).

One process, one context at a time: a context with n_owned < nv and no transport is legal, and fedm_set_state with
u_new takes the caller's ghost values as they are, so every rank of a partition can be created here in turn and given
the global states restricted to its vertices.  Such a context takes launch forms no one-GPU test reaches: the facets in
boundary_kernel<.., ATOMIC> followed by dirichlet_kernel instead of the fused facet/Dirichlet kernel, identity rows on
the ghosts of a one-layer halo or on the listed outermost layer of a deep one, redundantly assembled ghost rows.

Per (model, partition), for depth in (1, 3, 8) and every rank: F of residual() on every local row, J of two Jacobian
assemblies in a row, the F the F + J assembly leaves, the product, and fnorm -- against what
rank_assembly_reference.expected_local_system cuts out of the restatement's global F and J.

Row sets the library documents for a context without transport, asserted as such:
  * fnorm is the norm over the owned rows (Ctx::n_dot = n_owned * n_eq): one rank's term of the all-reduced sum.
  * the product writes the owned rows only ("ghost / padding rows belong to someone else", spmv.hip): rows of ghost
    vertices come out exactly 0, the assembled ones included.  What the redundantly assembled ghost rows would
    multiply to is checked on the host, jacobian_csr() @ x against the global J x on every assembled row.

Tolerances: those of tests/test_gpu_wall_flux.py and tests/test_gpu_tabulated.py for two implementations of the same
tensors -- F 1e-11 of max |F_global|, J 1e-10 of each row's largest entry, product 1e-11 of max |J x|, fnorm rel 1e-11;
identity rows exactly 0 and 1.

Measured on an MI355X (largest over the ranks: F, J, product; per depth 1 | 3 | 8); every test below runs in under
0.1 s once the first context of the process exists (1.9 s):
  streamer (lds-patches/one-pass)  r-cut  1.1e-12 1.6e-14 6.2e-15 | 1.1e-12 1.6e-14 6.2e-15 | 1.1e-12 1.6e-14 6.2e-15
                                   z-cut  5.3e-13 1.6e-14 5.2e-15 | 5.3e-13 1.6e-14 5.2e-15 | 1.1e-12 1.6e-14 6.4e-15
                                   three  1.1e-12 1.6e-14 6.2e-15 | 1.1e-12 1.6e-14 6.2e-15 | 1.1e-12 1.6e-14 6.4e-15
  tabulated (lds-patches)          r-cut  1.1e-12 1.6e-14 6.2e-15 | 1.1e-12 1.6e-14 6.4e-15 | 1.1e-12 1.6e-14 6.2e-15
                                   z-cut  5.3e-13 1.6e-14 5.2e-15 | 5.3e-13 1.6e-14 5.2e-15 | 1.1e-12 1.6e-14 6.4e-15
                                   three  1.1e-12 1.6e-14 6.4e-15 | 1.1e-12 1.6e-14 6.4e-15 | 1.1e-12 1.6e-14 6.4e-15
  walls (lds-patches)              r-cut  5.7e-13 1.3e-14 6.3e-15 | 5.7e-13 1.3e-14 6.3e-15 | 5.7e-13 1.3e-14 6.3e-15
                                   z-cut  7.0e-13 1.5e-14 7.3e-15 | 7.0e-13 1.5e-14 7.5e-15 | 7.0e-13 1.5e-14 7.5e-15
                                   three  3.5e-13 1.3e-14 5.8e-15 | 3.5e-13 1.3e-14 5.8e-15 | 7.0e-13 1.5e-14 7.5e-15
  walls (global colouring)         all    1.3e-12 1.1e-14 5.1e-15 at every depth
Before Dirichlet dofs of identity vertices were taken out of dirichlet_kernel's rows, the r-cut and three cases of all
four models failed at depth 3 (the first deep halo of the loop, where a test stops) on F of exactly those dofs (u - value instead of 0, e.g. 707.15 and 2286.03 on
rank 0 of the r-cut); the z-cut cases, which have no such dof, passed.
"""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import rank_assembly_reference as rr

pytestmark = pytest.mark.gpu

NEQ = 3
PARTITIONS = ("r-cut", "z-cut", "three")


def _rel_rows(A, B):
    D = abs(A - B)
    scale = np.maximum(abs(B).max(axis=1).toarray().ravel(), 1e-300)
    return (sp.diags(1.0 / scale) @ D).max()


@pytest.fixture(scope="module")
def setup():
    """The mesh, its partitions and local meshes, and per model the restatement's global F, J and J x (computed once,
    never changed)."""
    msh = rr.mesh()
    parts = rr.partitions(msh.coords, msh.cells)
    lms = {(name, depth): rr.local_meshes(msh.coords, msh.cells, part, depth)
           for name, part in parts.items() for depth in rr.DEPTHS}
    cases = {}
    for name, make in rr.CASES.items():
        c = make(msh)
        c["x"] = np.random.default_rng(5).normal(size=c["F"].size)
        c["Jx"] = c["J"] @ c["x"]
        cases[name] = c
    return dict(mesh=msh, lms=lms, cases=cases)


def _create(msh, lm, model):
    from fedm_amd.device import DeviceProblem
    dofs, vals = rr.local_dirichlet(lm, model.n_eq)
    return DeviceProblem(lm.coords, lm.cells, model, facet_tags=rr.local_facet_tags(msh, lm), dirichlet_dofs=dofs,
                         dirichlet_vals=vals, n_owned=lm.n_owned,
                         identity_vertices=lm.identity_vertices if lm.depth > 1 else None, halo_depth=lm.depth)


def _one_rank(msh, c, lm, what, not_one_pass):
    """One context: everything compared, the figures printed first.  Returns the launched Jacobian variant."""
    F_exp, J_exp, assembled = rr.expected_local_system(lm, c["F"], c["J"], NEQ)
    ident = np.nonzero(~assembled)[0]
    n_own = lm.n_owned * NEQ
    gdof = (lm.vertex_global[:, None] * NEQ + np.arange(NEQ)[None, :]).ravel()
    Fscale, Pscale = np.abs(c["F"]).max(), np.abs(c["Jx"]).max()
    x_loc, y_exp = c["x"][gdof], c["Jx"][gdof]
    prob = _create(msh, lm, c["model"]())
    try:
        prob.set_state(*[rr.restrict(lm, U) for U in c["states"]])
        prob.set_step(*rr.DT)
        F_gpu, fnorm = prob.residual()
        eF = np.abs(F_gpu - F_exp).max() / Fscale
        eJ, J_gpu = [], None
        for _ in range(2):      # a kept plane that the facets add to shows on the second assembly
            prob.jacobian()
            J_gpu = prob.jacobian_csr()
            eJ.append(_rel_rows(J_gpu, J_exp))
        F_fj = prob.residual_vector()
        eFJ = np.abs(F_fj - F_exp).max() / Fscale
        launched = prob.launched_assembly()
        y = prob.spmv(x_loc)
        eP = np.abs(y[:n_own] - y_exp[:n_own]).max() / Pscale
        eP_host = np.abs((J_gpu @ x_loc - y_exp)[assembled]).max() / Pscale
        fn_exp = np.linalg.norm(F_exp[:n_own])
        print(f"[rank assembly] {what} rank {lm.rank} ({lm.n_owned} owned + {lm.n_ghost} ghost): F {eF:.2e} "
              f"F of F+J {eFJ:.2e} J {eJ[0]:.2e} {eJ[1]:.2e} product {eP:.2e} host product {eP_host:.2e} "
              f"fnorm rel {abs(fnorm - fn_exp) / fn_exp:.2e} launched {launched['residual']['variant']} / "
              f"{launched['jacobian']['variant']}", flush=True)
        for kind in ("residual", "jacobian"):
            assert launched[kind]["variant"] is not None
            if not_one_pass:
                assert launched[kind]["variant"] != "lds-patches/one-pass", (what, kind)
        # identity rows: exactly 0 and 1 (a Dirichlet dof on such a row included)
        bad = ident[(F_gpu[ident] != 0.0) | (F_fj[ident] != 0.0)]
        assert bad.size == 0, (what, lm.rank, "F on identity rows (local dof, vertex layer)",
                               [(int(d), int(lm.layer[d // NEQ]), float(F_gpu[d]), float(F_fj[d])) for d in bad])
        Ji = J_gpu[ident]
        Ji.eliminate_zeros()
        assert Ji.nnz == ident.size and np.array_equal(Ji.indices, ident) and np.all(Ji.data == 1.0), (what, lm.rank)
        assert eF < 1e-11 and eFJ < 1e-11, (what, lm.rank, eF, eFJ)
        assert max(eJ) < 1e-10, (what, lm.rank, eJ)
        assert eP < 1e-11 and eP_host < 1e-11, (what, lm.rank, eP, eP_host)
        assert np.all(y[n_own:] == 0.0), (what, lm.rank)       # the product's documented row set: owned rows
        assert fnorm == pytest.approx(fn_exp, rel=1e-11), (what, lm.rank)
        return launched["jacobian"]["variant"], prob.plane_masks()
    finally:
        prob.close()


def _all_depths_and_ranks(setup, model, partition, not_one_pass):
    msh, c = setup["mesh"], setup["cases"][model]
    t0, variants, masks = time.time(), set(), set()
    for depth in rr.DEPTHS:
        for lm in setup["lms"][partition, depth]:
            v, m = _one_rank(msh, c, lm, f"{model} {partition} depth {depth}", not_one_pass)
            variants.add(v)
            masks.add(m)
    print(f"[rank assembly] {model} {partition}: variants {sorted(variants)}, {time.time() - t0:.1f} s", flush=True)
    return variants, masks


@pytest.mark.parametrize("partition", PARTITIONS)
def test_streamer_on_a_rank(setup, partition):
    """(a) cases.streamer.model() against oracle.streamer.build.  Whatever volume kernel the dispatch picks for a
    context with ghosts (the printed line names it) must hold the tolerances."""
    _all_depths_and_ranks(setup, "streamer", partition, not_one_pass=False)


@pytest.mark.parametrize("partition", PARTITIONS)
def test_tabulated_streamer_on_a_rank(setup, partition):
    """(b) mu_e, D_e and the ionisation rate as tables, knots from the quantiles of the global |E|."""
    _all_depths_and_ranks(setup, "tabulated", partition, not_one_pass=True)


@pytest.mark.parametrize("partition", PARTITIONS)
def test_walls_on_a_rank(setup, partition):
    """(c) 'flux source' walls: the WALL twin of the atomic facet kernel, wall terms that read the potential at ghost
    vertices; the state is off the Dirichlet values, so F of a Dirichlet dof on an identity vertex tells 0 (the
    identity row it must be) from u - value.  The plane masks are the one-GPU context's on the whole mesh, the
    emission plane (bit 3) neither kept nor skipped."""
    import wall_flux_reference as wr
    msh = setup["mesh"]
    whole = wr.device_problem(msh.coords, msh.cells, wr.device_two_species_model())
    try:
        masks_whole = whole.plane_masks()
    finally:
        whole.close()
    _, masks = _all_depths_and_ranks(setup, "walls", partition, not_one_pass=True)
    assert masks == {masks_whole}, (masks, masks_whole)
    assert masks_whole[1] & 8 == 0


@pytest.mark.parametrize("depth", rr.DEPTHS)
def test_new_dirichlet_values_reach_their_rows_on_a_rank(setup, depth):
    """set_dirichlet_values on a context whose Dirichlet list holds dofs of identity vertices (r-cut: two per rank, the
    cathode's among the entries before the anode's): the values are the caller's, in the caller's order; F of
    an assembled Dirichlet row is u - value exactly, identity rows stay 0, every other row is unchanged."""
    msh, c = setup["mesh"], setup["cases"]["walls"]
    for lm in setup["lms"]["r-cut", depth]:
        F_exp, _, assembled = rr.expected_local_system(lm, c["F"], c["J"], NEQ)
        dofs, vals = rr.local_dirichlet(lm, NEQ)
        on_identity = ~assembled[dofs]
        assert on_identity.sum() == 2 and on_identity[:-2].any()        # not both at the list's end already
        new = vals + 100.0 + 7.0 * np.arange(vals.size)
        u = rr.restrict(lm, c["states"][0]).ravel()
        F_exp[dofs[~on_identity]] = u[dofs[~on_identity]] - new[~on_identity]
        prob = _create(msh, lm, c["model"]())
        try:
            prob.set_state(*[rr.restrict(lm, U) for U in c["states"]])
            prob.set_step(*rr.DT)
            prob.set_dirichlet_values(new)
            F_gpu, _ = prob.residual()
        finally:
            prob.close()
        assert np.array_equal(F_gpu[dofs], F_exp[dofs]), (depth, lm.rank, F_gpu[dofs] - F_exp[dofs])
        assert np.all(F_gpu[~assembled] == 0.0)
        assert np.abs(F_gpu - F_exp).max() < 1e-11 * np.abs(c["F"]).max()


@pytest.mark.parametrize("partition", PARTITIONS)
def test_walls_on_a_rank_coloured(setup, partition, monkeypatch):
    """(d) FEDM_ASSEMBLY=colour: coloured facets, plain adds, no atomics."""
    monkeypatch.setenv("FEDM_ASSEMBLY", "colour")
    variants, _ = _all_depths_and_ranks(setup, "walls", partition, not_one_pass=True)
    assert variants == {"global colouring"}
