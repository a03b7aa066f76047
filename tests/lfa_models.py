"""Device contexts of LFA models other than the benchmark deck's, shared by the GPU tests (helper module)."""
import numpy as np


def four_species_problem(n=20, grading=2.0, oracle_model=True):
    """The largest model `fedm_model_desc` holds (FEDM_MAX_SPECIES = 4 + Poisson, five equations) on the graded n x n
    streamer mesh (20 x 20 unless told otherwise; oracle_model=False: without the oracle's model, None in its place --
    what a large mesh wants): a metastable that only diffuses, an ion that drifts, a negative ion drifting with a
    prescribed velocity, electrons with field-dependent coefficients; three reactions with field-dependent, constant
    and quadratic rates.  Returns (mesh, device problem, the oracle's model of it, Dirichlet dofs, Dirichlet values)."""
    from oracle import streamer as ost
    from oracle.forms import LFAModel
    from oracle.mesh import Mesh as OMesh, mark_boundaries
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum, parse
    msh = streamer.mesh(n, grading)
    m = Mesh(msh.coords, msh.cells)
    tags = Marking_boundaries(m, streamer.BOUNDARIES)
    eq = ["diffusion-reaction", "drift-diffusion-reaction", "drift-diffusion-reaction", "drift-diffusion-reaction"]
    Z = [0.0, 1.0, -1.0, -1.0]
    bc = [[kind[0]] * 3 + [kind[1]] for kind in streamer.BC_TYPE]        # the electrons keep the deck's wall types
    mu_e = parse(streamer.MU_E)
    ionisation = parse(streamer.ALPHA) * mu_e * TermSum.field()
    model = Model(n_species=4, poisson=True, eq_type=eq, Z=Z,
                  mu=[TermSum.const(0.0), TermSum.const(2e-4), TermSum.const(0.0), mu_e],
                  D=[TermSum.const(5e-4), TermSum.const(3e-6), TermSum.const(2e-3), parse(streamer.D_E)],
                  reactions=[Reaction(ionisation, power=[0, 0, 0, 1], net=[0, 1, 0, 1]),
                             Reaction(TermSum.const(3e-17), power=[1, 0, 0, 1], net=[-1, 1, 0, 1]),
                             Reaction(TermSum.const(1e-19), power=[0, 1, 1, 0], net=[1, -1, -1, 0])],
                  drift_w=[None, None, (1.0e3, -2.0e3), None], bc_kind=bc, quadrature_degree=2)
    ddofs, dvals = streamer.dirichlet(m.coords)
    ddofs = (ddofs // 3) * 5 + 4
    prob = DeviceProblem(m.coords, m.cells, model, facet_tags=tags, dirichlet_dofs=ddofs.astype(np.int32), dirichlet_vals=dvals)
    if not oracle_model:
        return m, prob, None, ddofs, dvals
    omesh = OMesh(msh.coords, msh.cells)
    om = LFAModel(omesh, 4, True, eq, Z,
                  mu=[0.0, 2e-4, 0.0, ost.MU_E], D=[5e-4, 3e-6, 2e-3, ost.D_E],
                  drift_w=[None, None, (1.0e3, -2.0e3), None],
                  reactions=[(ost.K_ION, [0, 0, 0, 1], [0, 1, 0, 1]), (3e-17, [1, 0, 0, 1], [-1, 1, 0, 1]),
                             (1e-19, [0, 1, 1, 0], [1, -1, -1, 0])],
                  facet_tags=mark_boundaries(omesh, ost.BOUNDARIES), bc_type=bc, qdeg=2)
    om.dirichlet_dofs, om.dirichlet_vals = ddofs.astype(np.int64), dvals
    return m, prob, om, ddofs, dvals


def recombining_streamer_problem(coords, cells):
    """The streamer model with electron-ion recombination added: both off-diagonal species planes of the Jacobian are
    nonzero (the ionisation couples the ions to the electrons, the recombination the electrons to the ions), so no
    species plane is structurally zero."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum, parse
    msh = Mesh(coords, cells)
    mu = parse(streamer.MU_E)
    model = Model(n_species=2, poisson=True, eq_type=["reaction", "drift-diffusion-reaction"], Z=[1.0, -1.0],
                  mu=[TermSum.const(0.0), mu], D=[TermSum.const(0.0), parse(streamer.D_E)],
                  reactions=[Reaction(parse(streamer.ALPHA) * mu * TermSum.field(), power=[0, 1], net=[1, 1]),
                             Reaction(TermSum.const(2e-13), power=[1, 1], net=[-1, -1])],
                  bc_kind=streamer.BC_TYPE, quadrature_degree=2)
    dofs, vals = streamer.dirichlet(msh.coords)
    return DeviceProblem(msh.coords, msh.cells, model, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                         dirichlet_dofs=dofs, dirichlet_vals=vals)
