"""The numpy restatement of the dielectric layers (tests/dielectric_reference.py) on the CPU: its Jacobian against finite
differences, the series-capacitor divider, the preconditions the GPU comparison rests on, that each deliberate fault
would miss the GPU tests' bounds by more than a factor of 100, and the conservation of plasma + surface charge.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import dielectric_reference as dr
import wall_flux_reference as wr
from oracle.forms import elementary_charge, epsilon_0

DT = (5e-12, 4e-12)
# the GPU tests' bounds (tests/test_gpu_dielectric.py: those of test_gpu_wall_flux.py, and the accept's)
BOUND_F, BOUND_J, BOUND_P, BOUND_Q = 1e-11, 1e-10, 1e-11, 1e-12
# ... and one bound more, on the Poisson rows of the layer vertices alone.  At the test states (n ~ 1e13 at the walls,
# dt = 5e-12) the mirrored entries are some 1e-9 of their row, so BOUND_J sees a fault in them 30 to 100 bounds away
# only.  An entry of these rows is a sum of at most a dozen products (two cells, two facet points, three species
# terms) of factors that the two implementations form with correctly rounded arithmetic and exp / pow a few ulp
# apart: 50 eps = 6e-15 of the row's largest entry at the most, and 1e-12 leaves a factor of 200 over that.
BOUND_J_LAYER = 1e-12


def component_error(a, b, neq):
    """max |a - b| per component over that component's max |b|: the Poisson row on its own scale"""
    a, b = a.reshape(-1, neq), b.reshape(-1, neq)
    return float((np.abs(a - b).max(axis=0) / np.abs(b).max(axis=0)).max())


def row_error(A, B):
    scale = np.maximum(abs(B).max(axis=1).toarray().ravel(), 1e-300)
    return float((sp.diags(1.0 / scale) @ abs(A - B)).max())


def layer_row_error(A, B, om):
    """row_error on the Poisson rows of the layer vertices that are no Dirichlet rows"""
    rows = np.setdiff1d(om.layer_vertices * om.neq + om.neq - 1, om.dirichlet_dofs)
    return row_error(A[rows], B[rows])


def _mesh():
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Mesh
    m = streamer.mesh(20, 2.0)
    msh = Mesh(m.coords, m.cells)
    return OMesh(msh.coords, msh.cells)


@pytest.fixture(scope="module")
def cases():
    """Per configuration: the restatement with a random charge history, the states, its F and J."""
    out = {}
    mesh = _mesh()
    for config in dr.CONFIGS:
        om = dr.oracle_two_species(mesh, config)
        U = wr.wall_state(mesh.coords)
        rng = np.random.default_rng(3)
        Uo, Uo1 = U - 0.01 * rng.random(U.shape), U - 0.02 * rng.random(U.shape)
        om.q, om.q_old = dr.random_history(om)
        F, J = om.residual_jacobian(U, Uo, Uo1, *DT)
        out[config] = dict(om=om, mesh=mesh, states=(U, Uo, Uo1), F=F, J=J)
    return out


@pytest.mark.parametrize("config", list(dr.CONFIGS))
def test_jacobian_against_finite_differences(cases, config):
    """Central differences along random directions, every row on its own scale.  Step 1e-6 in u: truncation ~1e-12
    relative, rounding ~1e-16/1e-6 times the cancellation in a row (the BDF term: ~1e2) -> 1e-6 is a safe bound."""
    c = cases[config]
    om, (U, Uo, Uo1) = c["om"], c["states"]
    rng = np.random.default_rng(8)
    worst = 0.0
    for _ in range(3):
        v = rng.normal(size=U.shape)
        v[:, 2] *= 1e-2 * np.abs(U[:, 2]).max()          # the potential's scale
        v.ravel()[om.dirichlet_dofs] = 0.0
        h = 1e-6
        Fp = om.residual(U + h * v, Uo, Uo1, *DT)
        Fm = om.residual(U - h * v, Uo, Uo1, *DT)
        fd, an = (Fp - Fm) / (2 * h), c["J"] @ v.ravel()
        scale = abs(c["J"]) @ np.abs(v.ravel())
        rows = scale > 0.0                                 # (Dirichlet rows in a direction that leaves them alone)
        worst = max(worst, float((np.abs(fd - an)[rows] / scale[rows]).max()))
        lv = om.layer_vertices * 3 + 2
        assert np.abs(an[lv]).max() > 0.0
    print(f"\n[dielectric] {config}: Jacobian against central differences {worst:.2e}")
    assert worst < 1e-6


@pytest.mark.parametrize("config", list(dr.CONFIGS))
def test_mirrored_jacobian_against_finite_differences(cases, config):
    """The mirror on its own scale.  In the full rows the mirrored entries are some 3e-9 of their row, below what the
    test above can see, so here the mirror's part of the Poisson rows, -kappa sum_s Z_s W_a,s(u), is formed directly
    (wall_moments: no cancellation) and differenced, against (J - J of the same model without layers - Robin mass) v
    on the layer's Poisson rows.  That matrix difference carries the rounding of the rows it is taken from, 1e-16 / 3e-9
    = 3e-8 of the mirrored entries; central differences with h = 1e-6 add 1e-10: 1e-5 leaves two orders over both, and a
    mirrored column that is missing or has the wrong factor is an error of order 1."""
    c = cases[config]
    om, (U, Uo, Uo1) = c["om"], c["states"]
    plain = wr.oracle_two_species(c["mesh"])
    _, Jp = plain.residual_jacobian(U, Uo, Uo1, *DT, apply_bc=False)
    _, Jl = om.residual_jacobian(U, Uo, Uo1, *DT, apply_bc=False)
    lv = om.layer_vertices
    rows = lv * 3 + 2
    R = sp.lil_matrix(Jl.shape)
    Rv = om.robin_matrix().tocoo()
    R[Rv.row * 3 + 2, Rv.col * 3 + 2] = Rv.data
    M = (Jl - Jp - R.tocsr())[rows]
    kappa = elementary_charge / epsilon_0 * om.step_coefficients(*DT)[2]
    mirror = lambda X: -kappa * om.wall_moments(X, *DT)[lv]       # noqa: E731
    rng = np.random.default_rng(9)
    worst = 0.0
    for _ in range(3):
        v = rng.normal(size=U.shape)
        v[:, 2] *= 1e-3 * np.abs(U[:, 2]).max()
        h = 1e-6
        fd, an = (mirror(U + h * v) - mirror(U - h * v)) / (2 * h), M @ v.ravel()
        scale = abs(M) @ np.abs(v.ravel())
        assert (scale > 0.0).all()
        # the potential column counts: its share of the product is not small
        vphi = np.zeros_like(v)
        vphi[:, 2] = v[:, 2]
        assert (np.abs(M @ vphi.ravel()) / scale).max() > 1e-2
        worst = max(worst, float((np.abs(fd - an) / scale).max()))
    print(f"\n[dielectric] {config}: the mirror's Jacobian against central differences {worst:.2e}")
    assert worst < 1e-5


def test_vacuum_divider():
    """Planar tensor mesh of height g, a layer on z = 0 with the conductor at U behind it, V on z = g, densities
    negligible and q = 0: the surface potential is U + (V - U) (d/eps_r)/(g + d/eps_r), and the restatement's Poisson
    rows are linear in Phi, so one dense solve from any start gives it to rounding."""
    from oracle.mesh import mark_boundaries, rectangle_right
    from oracle import streamer as ost
    g, V, U_l, d, eps_r = ost.BOX, 1000.0, 100.0, 2e-4, 5.0
    mesh = rectangle_right(0.0, 0.0, g, g, 6, 6)
    bc = [["zero flux", "zero flux"]] * 4
    om = dr.DielectricLFAModel(mesh, 2, True, ["drift-diffusion-reaction"] * 2, [1.0, -1.0], mu=[wr.MU_ION, ost.MU_E],
                               D=[wr.D_ION, ost.D_E], reactions=[], facet_tags=mark_boundaries(mesh, ost.BOUNDARIES),
                               bc_type=bc, qdeg=2, axisymmetric=False, walls=wr.two_species_walls(0.0),
                               layers={1: (d, eps_r, U_l)})
    top = np.nonzero(np.abs(mesh.coords[:, 1] - g) < 1e-14)[0]
    om.set_dirichlet(top * 3 + 2, np.full(top.size, V))
    Ustate = np.full((mesh.nv, 3), -200.0)                   # n = exp(-200): no charge
    Ustate[:, 2] = V * mesh.coords[:, 1] / g + 1.0           # any start with a field
    F, J = om.residual_jacobian(Ustate, Ustate, Ustate, 1e-12, 1e30)
    ip = np.arange(mesh.nv) * 3 + 2
    dphi = spla.spsolve(sp.csc_matrix(J[ip][:, ip]), -F[ip])
    phi = Ustate[:, 2] + dphi
    expect = U_l + (V - U_l) * (d / eps_r) / (g + d / eps_r)
    bottom = np.abs(mesh.coords[:, 1]) < 1e-14
    err = np.abs(phi[bottom] - expect).max() / abs(V)
    print(f"\n[dielectric] divider: surface potential {phi[bottom].mean():.9g}, expected {expect:.9g}, error {err:.2e}")
    assert err < 1e-12
    # ... and the layer's displacement charge is the capacitor's: eps0 eps_r/d (Phi_s - U) times the planar measure
    disp = om.displacement_charge(np.column_stack([Ustate[:, :2], phi]))[1]
    assert disp == pytest.approx(epsilon_0 * eps_r / d * (expect - U_l) * g, rel=1e-12)


@pytest.mark.parametrize("config", list(dr.CONFIGS))
def test_preconditions(cases, config):
    """On the layer vertices the surface-charge addend and the Robin addend each reach 2.5e-3 of the Poisson row's scale
    (tests/test_lmea_family_reference.py's threshold), and the wall flux takes both signs on the layer.  What that
    means per configuration, asserted as such: on r = BOX the deposited sum sum_s Z_s W_a,s itself changes sign along
    the layer (the electrons' drift term follows E.n).  On the cathode it does NOT: at the test states the net deposit
    has the electrons' sign at every vertex (vth_e is 250 vth_i at equal densities); there the two signs are those of
    the species' own moments Z_s W_a,s, the ions' against the electrons', which is what exercises Z_s in the mirror."""
    c = cases[config]
    om, (U, Uo, Uo1) = c["om"], c["states"]
    wr.assert_preconditions(om, U)
    rows = om.layer_vertices * 3 + 2
    free = np.setdiff1d(rows, om.dirichlet_dofs)
    F_all = om.residual(U, Uo, Uo1, *DT, apply_bc=False)
    scale = np.abs(F_all[2::3]).max()
    # the addends, by taking them out one at a time
    plain = wr.WallLFAModel(om.mesh, 2, True, om.eq_type, om.Z, mu=om.mu, D=om.D, reactions=om.reactions,
                            facet_tags=om.facet_tags, bc_type=om.bc_type, qdeg=2, walls=dict(om.walls))
    F_plain = plain.residual(U, Uo, Uo1, *DT, apply_bc=False)
    Re = np.zeros((om.mesh.nc, 3, 3))
    om._robin(U[om.mesh.cells], Re, None)
    robin = om._scatter_vec(Re)
    charge = (F_all - F_plain) - robin
    moments = om.wall_moments(U, *DT)[om.layer_vertices]
    per_species = np.concatenate([om.Z[s] * om._scatter_vec(om._layer_R * (np.arange(3) == s))[s::3][om.layer_vertices]
                                  for s in range(2)])
    r_robin, r_charge = np.abs(robin[free]).max() / scale, np.abs(charge[free]).max() / scale
    print(f"\n[dielectric] {config}: Robin addend {r_robin:.2e}, surface-charge addend {r_charge:.2e} of the Poisson row's "
          f"scale; wall moments {moments.min():.2e} .. {moments.max():.2e}")
    assert r_robin >= 2.5e-3 and r_charge >= 2.5e-3
    assert (per_species > 0).any() and (per_species < 0).any()
    if config == "outer":
        assert (moments > 0).any() and (moments < 0).any()
    else:
        assert (moments < 0).all()


# the fault -> the comparison of the GPU tests that is meant to catch it, and the configurations it shows in
CAUGHT_BY = {"Z dropped from the mirror": ("J", ("cathode", "outer")),
             "history left out": ("F", ("cathode", "outer")),
             "w^2 taken as w": ("F", ("cathode", "outer")),
             "potential column not mirrored": ("J_layer", ("cathode", "outer")),
             "Robin term without U": ("F", ("cathode", "outer")),
             "emission not deposited": ("J_layer", ("cathode",))}
assert set(CAUGHT_BY) == set(dr.FAULTS)


@pytest.mark.parametrize("fault", dr.FAULTS)
def test_each_fault_misses_the_gpu_bounds(cases, fault):
    """What the GPU tests compare (F and the product per component, J per row, the layer's Poisson rows of J, the
    accepted q) with the fault built in,
    against the restatement without it: the metric that is meant to catch the fault (CAUGHT_BY) misses its bound by
    more than a factor of 100, in every configuration the fault shows in (the secondaries: on the cathode alone)."""
    metric, configs = CAUGHT_BY[fault]
    for config in configs:
        c = cases[config]
        om, (U, Uo, Uo1) = c["om"], c["states"]
        bad = dr.oracle_two_species(c["mesh"], config, fault=fault)
        bad.q, bad.q_old = om.q.copy(), om.q_old.copy()
        F, J = bad.residual_jacobian(U, Uo, Uo1, *DT)
        x = np.random.default_rng(5).normal(size=F.size)
        q_ok, q_bad = om.charge(U, *DT), bad.charge(U, *DT)
        miss = dict(F=component_error(F, c["F"], 3) / BOUND_F, J=row_error(J, c["J"]) / BOUND_J,
                    J_layer=layer_row_error(J, c["J"], om) / BOUND_J_LAYER,
                    product=component_error(J @ x, c["J"] @ x, 3) / BOUND_P,
                    q=np.abs(q_bad - q_ok).max() / np.abs(q_ok).max() / BOUND_Q)
        print(f"\n[dielectric] fault '{fault}', {config}: bounds missed by " + ", ".join(f"{k} {v:.1e}" for k, v in miss.items()))
        assert miss[metric] > 100.0, (config, metric, miss)


CONSERVATION_BC = [["flux source", "flux source"], ["zero flux"] * 2, ["zero flux"] * 2, ["zero flux"] * 2]


def conservation_case(mesh):
    """The restatement and the start of the conservation runs (this file's and tests/test_gpu_dielectric.py's): the
    linear representation, the layer on the cathode the only boundary with a species flux, a uniform field."""
    om = dr.oracle_two_species(mesh, "cathode", bc_type=CONSERVATION_BC, log=False)
    U0 = wr.wall_state(mesh.coords, log=False)
    U0[:, 2] = 18750.0 * mesh.coords[:, 1] / mesh.coords[:, 1].max()
    return om, U0


class ChargeLedger:
    """Q = e sum_s Z_s N_s + sum_a q_a along a run, and the bound on its drift.  Summing the species rows over all
    vertices (the flux term drops out, the ionisation makes pairs) gives BDF2(Q) = e sum_s Z_s sum_a F_a,s: the drift
    per step is at most cdt e sum_s |sum_a F_a,s| of the converged Newton residual -- the restatement's, at whatever
    state the step ended with -- carried on by the recurrence a1 Q_n - a2 Q_(n-1), whose roots are 1 and at most 1/3 in
    magnitude here (a factor 1.5), plus the rounding of the sums that make Q (64 eps of their absolute terms a step)."""

    def __init__(self, om, U0, q0):
        self.om, self.Q0 = om, om.species_charge(U0) + q0.sum()
        self.terms = self._terms(U0, q0)
        self.bound, self.drift, self.steps = 0.0, [], 0

    def _terms(self, U, q):
        om = self.om
        return sum(abs(om.species_charge(np.column_stack([U[:, :2] * (np.arange(2) == s), U[:, 2]]))) for s in range(2)) \
            + np.abs(q).sum()

    def step(self, U, Uo, Uo1, dt, dt_old, q):
        """after the step to U was solved and its charge q accepted"""
        F = self.om.residual(U, Uo, Uo1, dt, dt_old, apply_bc=False).reshape(-1, 3)
        cdt = self.om.step_coefficients(dt, dt_old)[2]
        self.bound += 1.5 * cdt * elementary_charge * sum(abs(F[:, s].sum()) for s in range(2))
        self.terms = max(self.terms, self._terms(U, q))
        self.drift.append(self.om.species_charge(U) + q.sum() - self.Q0)
        self.steps += 1

    @property
    def rounding(self):
        return 64 * np.finfo(float).eps * self.terms * self.steps

    def check(self, what, q):
        worst = np.abs(self.drift).max()
        print(f"\n[dielectric] conservation {what}: Q0 {self.Q0:.6e} C, surface charge {q.sum():.3e} C, drift {worst:.3e} C, "
              f"bound from the Newton residuals {self.bound:.3e} C + rounding {self.rounding:.3e} C", flush=True)
        assert abs(q.sum()) > 1e3 * (self.bound + self.rounding)          # the layer did take charge
        assert worst <= self.bound + self.rounding


def test_charge_conservation():
    """Every species-flux boundary is the layer or zero flux; five steps with unequal dt.  The scheme conserves
    Q = e sum_s Z_s N_s + sum_a q_a where the time term is the BDF2 quotient of the densities themselves, i.e. in the
    linear representation (in the logarithmic one the time term is n BDF2(u), which conserves nothing discretely), so
    that is the representation here.  The bound: ChargeLedger."""
    from oracle.newton import newton_solve
    om, U0 = conservation_case(_mesh())
    Uo, Uo1, U = U0.copy(), U0.copy(), U0.copy()
    ledger, dt_old = ChargeLedger(om, U0, om.q), 1e30
    for dt in [2e-12, 3e-12, 2.5e-12, 4e-12, 3e-12]:
        newton_solve(om, U, Uo, Uo1, dt, dt_old, 1e-10, 25)
        om.accept(U, dt, dt_old)
        ledger.step(U, Uo, Uo1, dt, dt_old, om.q)
        Uo1, Uo, dt_old = Uo, U.copy(), dt
    ledger.check("restatement", om.q)


def test_facade_lowers_a_dielectric_layer():
    """Dielectric_layer added to the wall form of tests/test_wall_flux_reference.py: Model.dielectric and its
    descriptor; without the piece the model is the one it was; what the device cannot run is refused by name."""
    from test_wall_flux_reference import _wall_forms
    from fedm_amd import functions as ff
    from fedm_amd.cases import streamer
    from fedm_amd.forms import FiniteElement, FunctionSpace, Measure, MixedElement, TestFunctions, TrialFunction
    from fedm_amd.mesh import RectangleMesh
    mesh = RectangleMesh((0, 0), (0.0125, 0.0125), 4, 4)
    ME = FunctionSpace(mesh, MixedElement([FiniteElement()] * 3))
    u, v = TrialFunction(ME), TestFunctions(ME)
    dsm = Measure("ds", domain=mesh, subdomain_data=ff.Marking_boundaries(mesh, streamer.BOUNDARIES))
    plain, _, _ = ff.compile_forms(_wall_forms(mesh))
    assert plain.dielectric is None
    F = _wall_forms(mesh) + ff.Dielectric_layer(u[2], v[2], dsm(1), 1e-4, 4.0, voltage=25.0)
    m, _, tags = ff.compile_forms(F)
    assert tags is not None and m.dielectric.tags() == [1]
    dd = m.dielectric.to_c()
    assert [dd.is_layer[t] for t in range(4)] == [1, 0, 0, 0]
    assert (dd.thickness[0], dd.eps_r[0], dd.voltage[0]) == (1e-4, 4.0, 25.0)
    assert bytes(m.to_c()) == bytes(plain.to_c()) and bytes(m.walls_to_c()) == bytes(plain.walls_to_c())
    with pytest.raises(ValueError, match="tag 1.*u must be the potential"):
        ff.compile_forms(_wall_forms(mesh) + ff.Dielectric_layer(u[1], v[1], dsm(1), 1e-4, 4.0))
    with pytest.raises(ValueError, match="tag 1.*has a layer already"):
        ff.compile_forms(F + ff.Dielectric_layer(u[2], v[2], dsm(1), 2e-4, 4.0))
    with pytest.raises(ValueError, match="thickness must be a positive number"):
        ff.Dielectric_layer(u[2], v[2], dsm(1), 0.0, 4.0)
    with pytest.raises(ValueError, match="eps_r must be a positive number"):
        ff.Dielectric_layer(u[2], v[2], dsm(1), 1e-4, -1.0)


def _captured_form(example, tmp_path, **kw):
    """The form (and the Dirichlet conditions) an example hands to Problem(), without a device."""
    import importlib.util
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location(example + "_dielectric", root / "examples" / (example + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}

    class Stop(Exception):
        pass

    def capture(J, F, bcs):
        seen.update(F=F, bcs=bcs)
        raise Stop
    with pytest.raises(Stop):
        mod.main(output_dir=tmp_path, stop_before_device=capture, **kw)
    return seen["F"], seen["bcs"], mod


def test_the_example_lowers_its_dielectric_flag(tmp_path):
    """streamer_discharge.py --dielectric 1:1e-4:4: the layer on the cathode at the cathode's voltage, the cathode's
    Dirichlet condition gone; off by default the model and the conditions it had."""
    from fedm_amd import functions as ff
    F0, bcs0, _ = _captured_form("streamer_discharge", tmp_path / "off", cells=8, quiet=True)
    F1, bcs1, mod = _captured_form("streamer_discharge", tmp_path / "on", cells=8, quiet=True, dielectric="1:1e-4:4")
    m0, m1 = ff.compile_forms(F0)[0], ff.compile_forms(F1)[0]
    assert m0.dielectric is None and len(bcs0) == 2
    assert m1.dielectric.tags() == [1] and len(bcs1) == 1
    assert (m1.dielectric.thickness[1], m1.dielectric.eps_r[1], m1.dielectric.voltage[1]) == (1e-4, 4.0, 0.0)
    assert bytes(m1.to_c()) == bytes(m0.to_c())
    assert mod.parse_dielectric("2:5e-5") == (2, 5e-5, 1.0)
    F2, bcs2, _ = _captured_form("streamer_discharge", tmp_path / "anode", cells=8, quiet=True, dielectric="2:5e-5")
    assert ff.compile_forms(F2)[0].dielectric.voltage[2] == mod.Case().anode_voltage and len(bcs2) == 1
    for bad, kw in (("TAG:THICKNESS", dict(dielectric="1")), ("coupled step only", dict(dielectric="1:1e-4", coupling="uncoupled")),
                    ("needs --dielectric", dict(surface_charge_log=str(tmp_path / "q.log")))):
        with pytest.raises(ValueError, match=bad):
            mod.main(cells=8, quiet=True, output_dir=tmp_path / "bad", **kw)


def test_a_layer_in_an_lmea_form_is_refused(tmp_path):
    """A Dielectric_layer piece in the glow-discharge form: refused by name, not dropped."""
    import types
    from fedm_amd import functions as ff
    F, _, _ = _captured_form("glow_discharge", tmp_path, nx=6, ny=6)
    pieces = list(F.pieces)
    ff.compile_forms(ff.FormSum(pieces))                           # the form as it is lowers
    ds1 = types.SimpleNamespace(tag=1, subdomain_data=None)
    layer = ff.Dielectric_layer(types.SimpleNamespace(index=len(pieces)), None, ds1, 1e-4, 4.0)
    with pytest.raises(ValueError, match="Dielectric_layer on tag 1: the LMEA family has no dielectric layers"):
        ff.compile_forms(ff.FormSum(pieces + [layer]))
