"""Positive streamer in air (Bagheri et al. 2018) on the device path.

Counterpart of examples/streamer_discharge/fedm-streamer.py: same deck
(file_input/benchmark_model), same boundary list, boundary-condition table,
initial conditions, Dirichlet values and solver settings.  The reference's
mesh.xml is not in its checkout, so the mesh is ours (tensor-product, optional
geometric grading towards the axis).
"""
from pathlib import Path

import numpy as np

from ..device import DeviceProblem, Model, Reaction
from ..mesh import Marking_boundaries, Mesh, RectangleMesh, geometric_lines
from ..termsum import TermSum, parse

U_W = 18750.0                 # fedm-streamer.py:39
BOX = 0.0125                  # :96-97
BOUNDARIES = [["line", 0.0, 0.0, 0.0, BOX], ["line", BOX, BOX, 0.0, BOX],
              ["line", 0.0, BOX, 0.0, 0.0], ["line", 0.0, BOX, BOX, BOX]]          # :98-101
BC_TYPE = [["zero flux", "Neumann"], ["zero flux", "Neumann"],
           ["zero flux", "zero flux"], ["zero flux", "zero flux"]]                 # :103-107
DECK = Path(__file__).resolve().parents[2] / "decks" / "streamer_discharge" / "file_input"
# deck strings, transport_coefficients/{e_Nb,e_ND,alpha}.dat:12 (used when no deck dir is given)
MU_E = "2.3987*E_m**(-0.26)"
D_E = "4.3628e-3*E_m**(0.22)"
ALPHA = "(1.1944e6 + 4.3666e26 * E_m**(-3))*exp(-2.73e7/E_m)-340.75"
N0 = 760.0 * 3.21877e22       # gas number density at 760 Torr, 300 K [1/m^3]: what E/N tables are scaled with


def model(mu_e=MU_E, D_e=D_E, alpha=ALPHA, quadrature_degree=2):
    """LFA model of fedm-streamer.py:235-271."""
    mu = parse(mu_e)
    rate = parse(alpha) * mu * TermSum.field()          # alpha*mu[1]*E_m, :244-245
    return Model(n_species=2, poisson=True,
                 eq_type=["reaction", "drift-diffusion-reaction"], Z=[1.0, -1.0],
                 mu=[TermSum.const(0.0), mu], D=[TermSum.const(0.0), parse(D_e)],
                 reactions=[Reaction(rate, power=[0, 1], net=[1, 1])],
                 bc_kind=BC_TYPE, quadrature_degree=quadrature_degree)


def _deck_coefficient(kx, ky, dependence):
    """A transport coefficient as the deck readers return it: a number, a 'fun:E' string, or an E/N table
    (kx in Td, ky = N0 * coefficient), which the element kernels look up at the cell's own |E|."""
    if dependence == "E/N":
        return TermSum.table(np.asarray(kx, dtype=np.float64) * N0 * 1e-21, ky) / N0
    return TermSum.coerce(ky)


def model_from_deck(file_input=DECK, model_name="benchmark_model", quadrature_degree=2):
    """The same model configured the way the script does it (fedm-streamer.py:47-53,
    227-245): species list, particle properties and transport coefficients through the
    deck readers; the 'fun:E' strings are parsed, never eval'd.  ``tabulated_model`` holds the electrons'
    coefficients and alpha / N0 as `Dependence: E/N` tables (tools/make_tabulated_deck.py)."""
    from .. import file_io, functions
    file_io.files.file_input = Path(file_input)
    path = file_io.files.file_input / model_name
    n_species, species, prop_files, _ = file_io.read_speclist(path)
    M, sign = file_io.read_particle_properties(prop_files, model_name)
    n_species, n_eq, species, M, sign = functions.modify_approximation_vars(
        "LFA", n_species, species, M, sign)
    D_x, D_y, D_dep = file_io.read_transport_coefficients(species, "Diffusion", model_name)
    mu_x, mu_y, mu_dep = file_io.read_transport_coefficients(species, "mobility", model_name)
    mu = [_deck_coefficient(*xyd) for xyd in zip(mu_x, mu_y, mu_dep)]
    D = [_deck_coefficient(*xyd) for xyd in zip(D_x, D_y, D_dep)]
    alpha_file = path / "transport_coefficients" / "alpha.dat"
    if file_io.read_dependence(alpha_file) == "E/N":        # alpha / N0 against E/N
        (a_x,), (a_y,) = file_io.read_rate_coefficients([alpha_file], ["E/N"])
        alpha = TermSum.table(np.asarray(a_x, dtype=np.float64) * N0 * 1e-21, a_y) * N0
    else:
        alpha = parse(file_io.read_single_string(alpha_file))
    rate = alpha * mu[1] * TermSum.field()
    return Model(n_species=n_species, poisson=True,
                 eq_type=["reaction", "drift-diffusion-reaction"], Z=sign, mu=mu, D=D,
                 reactions=[Reaction(rate, power=[0, 1], net=[1, 1])],
                 bc_kind=BC_TYPE, quadrature_degree=quadrature_degree)


def mesh(n, grading=1.0):
    """n x n "right" mesh of the 1.25 cm box; grading>1 refines towards the axis."""
    x_lines = geometric_lines(BOX, n, grading) if grading != 1.0 else None
    return RectangleMesh((0.0, 0.0), (BOX, BOX), n, n, "right", x_lines=x_lines)


# the channel the streamer of this case travels in: from the seed at z = 1 cm towards the cathode,
# radius about 1 mm when it arrives (Bagheri et al. 2018, case 1)
CHANNEL = (0.0, 0.9e-3, 1.0e-3, 10.8e-3)           # (r0, r1, z0, z1) of the finest region


def refined_mesh(h_fine, growth=0.2, channel=CHANNEL, h_max=BOX / 12, n_levels=None, xml_path=None, retriangulate=True):
    """Locally refined unstructured mesh of the box: spacing ``h_fine`` in the streamer channel,
    growing with the distance from it (`fedm_amd.meshgen`): the stand-in for the reference's
    ``mesh.xml`` (fedm-streamer.py:116; missing from its checkout).  With ``xml_path`` the mesh
    is written as legacy DOLFIN XML and READ BACK through the reader a user mesh takes, so what
    the device gets went the way of ``Mesh('mesh.xml')``."""
    from .. import meshgen, mesh_io
    if n_levels is None:
        n_levels = max(2, int(np.ceil(np.log2(h_max / h_fine))) + 1)
    size = meshgen.box_distance_size(channel, h_fine, growth, h_max)
    msh = meshgen.refined_rectangle(BOX, BOX, size, h_fine, n_levels=n_levels, retriangulate=retriangulate)
    if xml_path is not None:
        mesh_io.write_dolfin_xml(msh, xml_path)
        msh = mesh_io.read_dolfin_xml(xml_path)
    return msh


def dirichlet(coords):
    """Phi = 0 at z = 0 and Phi = U_w at z = box height (fedm-streamer.py:186-200,233)."""
    z = coords[:, 1]
    cathode = np.nonzero(np.abs(z) < 3e-16)[0]
    anode = np.nonzero(np.abs(z - BOX) < 3e-16)[0]
    dofs = np.concatenate([cathode, anode]) * 3 + 2
    vals = np.concatenate([np.zeros(cathode.size), np.full(anode.size, U_W)])
    return dofs.astype(np.int32), vals


def initial_log_densities(coords):
    """fedm-streamer.py:169-172."""
    r, z = coords[:, 0], coords[:, 1]
    u_ion = np.log(1e13 + 5e18 * np.exp(-(r ** 2 + (z - 1e-2) ** 2) / (0.4e-3) ** 2))
    return u_ion, np.full_like(u_ion, np.log(1e13))


# Photoionisation (Bagheri et al. 2018, case 3): the three-term Helmholtz fit of Bourdon et al. 2007 and the case's
# efficiency, quoted from memory (check the papers before relying on a run; no test depends on these numbers):
# A [1/(cm^2 Torr^2)], lambda [1/(cm Torr)], p_O2 [Torr], efficiency xi p_q / (p + p_q)
PHOTO_A, PHOTO_LAMBDA, PHOTO_P_O2 = (1.986e-4, 0.0051, 0.4886), (0.0553, 0.1460, 0.89), 150.0
PHOTO_EFFICIENCY = 0.075 * 30.0 / (750.0 + 30.0)


def default_photoionization(**overrides):
    """The case's photoionisation source for ``device_problem(..., photoionization=...)``: the ionisation reaction
    (reaction 0) feeds it, ions and electrons receive it, the Helmholtz solutions vanish on the two electrodes
    (tags 1, 2)."""
    from ..device import Photoionization
    kw = dict(reactions=[0], efficiency=PHOTO_EFFICIENCY, c=[1e4 * a * PHOTO_P_O2 ** 2 for a in PHOTO_A],
              kappa=[1e2 * v * PHOTO_P_O2 for v in PHOTO_LAMBDA], targets=[0, 1], zero_tags=[1, 2])
    kw.update(overrides)
    return Photoionization(**kw)


def device_problem(coords, cells, device=0, deck_model=None, photoionization=None, dielectric=None, **model_kw):
    """``deck_model``: the model of that deck folder (``model_from_deck``: "benchmark_model", "tabulated_model")
    instead of the built-in strings.  ``photoionization``: a :class:`fedm_amd.device.Photoionization` (``True``: the
    case's own, :func:`default_photoionization`); None: none, as the benchmark's case 1.  ``dielectric``: a
    :class:`fedm_amd.device.Dielectric`; an electrode it coats (tag 1: the cathode, tag 2: the anode) loses its
    Dirichlet values -- the conductor is behind the layer, at the electrode's voltage unless the description names
    another; None: the path as it was."""
    import copy
    msh = Mesh(coords, cells)
    tags = Marking_boundaries(msh, BOUNDARIES)
    dofs, vals = dirichlet(msh.coords)
    lfa = model_from_deck(model_name=deck_model, **model_kw) if deck_model else model(**model_kw)
    if dielectric is not None:
        dielectric = copy.deepcopy(dielectric)      # (the caller's description stays as it was given)
        z = msh.coords[dofs // lfa.n_eq, 1]
        for tag, on, volts in ((1, np.abs(z) < 3e-16, 0.0), (2, np.abs(z - BOX) < 3e-16, U_W)):
            if tag in dielectric.thickness:
                dofs, vals, z = dofs[~on], vals[~on], z[~on]
                dielectric.voltage.setdefault(tag, volts)
    lfa.dielectric = dielectric
    if photoionization is not None and photoionization is not False:
        lfa.photoionization = default_photoionization() if photoionization is True else photoionization
    return DeviceProblem(msh.coords, msh.cells, lfa, facet_tags=tags,
                         dirichlet_dofs=dofs, dirichlet_vals=vals, device=device)


def diagnostics(prob):
    """The case's own diagnostics set-up on ``prob`` (``fedm_amd.functions.Discharge_diagnostics``): the head is the
    field maximum among the cells nearer to the axis than the channel radius the refinement uses, psi = z / BOX (exact
    for the planar gap), group 0 the cathode (tag 1), group 1 the anode (tag 2).  Returns the callable."""
    from ..functions import Discharge_diagnostics
    return Discharge_diagnostics(prob, boundary_tags=(1, 2), window=(0.0, CHANNEL[1], 0.0, BOX),
                                 weighting_potential=prob.coords[:, 1] / BOX)


SPECIES_NAMES = ("ions", "electrons")        # the model's species order (fedm-streamer.py:60)

DIAGNOSTIC_COLUMNS = ("t", "z_head", "E_max_axis", "E_max", "N_i", "N_e", "net_charge", "surface_charge_cathode",
                      "surface_charge_anode", "current", "ni_max", "ne_max")


# V(1,1): as effective as V(2,2) here at 75 % of the cost; Jacobi damping 0.85 instead of the
# default 2/3: the same 6 Krylov steps per time step early in the run, 35 instead of 38 later
# (tools/omega_sweep.py; 0.95: 40)
# V(1,1) with damped Jacobi; next to it a cycle with two Chebyshev sweeps per leg for the Newton
# solves that need many Krylov steps (once the streamer has formed: 27 instead of 37 Krylov steps
# per time step for 29 us more per cycle, tools/poly_cycle.py)
MULTIGRID = dict(nu=1, omega=0.85, hard_poly_degree=2)


def initialise(prob, multigrid=True):
    """Initial densities + the initial Poisson solve (fedm-streamer.py:169-225) on the device."""
    U = np.zeros((prob.nv, 3))
    U[:, 0], U[:, 1] = initial_log_densities(prob.coords)
    prob.set_state(U, U, U)
    if multigrid:
        prob.setup_multigrid(**MULTIGRID)
        # species block ~ diagonally scaled P1 mass matrix (spectrum in [0.5, 2]): a Chebyshev
        # polynomial in Duu^-1 Juu instead of plain block Jacobi.  Degree 6 makes a Newton system
        # cost 2 Krylov steps early in the run (degree 4: 3, block Jacobi: 5); later the potential
        # block limits the convergence (8-9 steps whatever the degree) and degree 4 is cheaper:
        # the library switches on the iteration count (tools/fs_sweeps.py).  (The potential-first
        # order of the split halves the late count but not the error: tools/fs_order_accuracy.py.)
        from ..device import chebyshev_weights
        prob.set_fieldsplit(chebyshev_weights(6), hard_weights=chebyshev_weights(4))
    its = prob.poisson_solve(rtol=1e-12)
    U = prob.get_state()
    prob.set_state(U, U, U)
    return U, its



class Stepper:
    """The script-level time loop of fedm-streamer.py:304-340 around one device problem."""

    partition_name = "single GPU"

    @property
    def assembly_kernel_name(self):
        sz = self.prob.sizes()
        if sz["assembly_variant"] == "lds-patches/one-pass":
            return (f"assemble_lean3_kernel<2,1,{sz['patch_threads']},kept planes> (LDS patches with micro-coloured cell "
                    "order, one pass over the cells, live planes only, F+J)")
        if sz["assembly_variant"] != "lds-patches":
            return f"volume assembly, variant '{sz['assembly_variant']}' (F+J)"
        return (f"assemble_lean2_kernel<2,1,{sz['patch_threads']}> (LDS patches with micro-coloured cell order, one "
                "equation row at a time, F+J)")

    @property
    def multigrid_levels(self):
        return getattr(self.prob, "multigrid_levels", None)

    def __init__(self, prob, dt_init=5e-12, dt_max=5e-12, dt_min=1e-15, ttol=1e-3,
                 relative_tolerance=1e-4, maximum_iterations=20, error_file=None, quiet=True,
                 coupling="coupled", circuit=None):
        import tempfile
        from .. import functions as ff
        from ..forms import DeviceState, Expression, FunctionAssigner
        self.ff, self.prob = ff, prob
        self.solver = ff.PETScSNESSolver()
        self.solver.parameters["relative_tolerance"] = relative_tolerance
        self.solver.parameters["maximum_iterations"] = maximum_iterations
        self.solver.parameters["coupling"] = coupling      # "uncoupled": the segregated step (PETScSNESSolver)
        self.problem = ff.Problem(None, None, [], device_problem=prob)
        self.dt = Expression("time_step", time_step=dt_init, degree=0)
        self.dt_old = Expression("time_step", time_step=1e30, degree=0)
        self.u_new, self.u_old = DeviceState(prob, "new"), DeviceState(prob, "old")
        self.assigner = FunctionAssigner()
        self.error, self.max_error = [0.0] * 2, [1] * 3
        self.ttol, self.dt_min, self.dt_max = ttol, dt_min, dt_max
        if error_file is None:
            error_file = Path(tempfile.mkdtemp(prefix="fedm_amd_")) / "relative error.log"
        self.error_file = Path(error_file)
        open(self.error_file, "w").close()
        self.t, self.steps, self.newton_iterations, self.linear_iterations = 0.0, 0, 0, 0
        self.quiet = quiet
        self.total_dofs = prob.n
        # circuit: dict(resistance=ohms, capacitance=farads) -- the anode behind a series resistor with a stray capacitance
        # to ground (fedm.External_circuit; the cathode stays an ideal ground), advanced before every solve attempt;
        # None: the ideal source, as ever.  Set up at the first step, once the initial state stands.
        self._circuit_spec, self.circuit, self._timed = circuit, None, []

    def _circuit_setup(self):
        spec = self._circuit_spec
        self.currents()             # (sets the electrodes up)
        self.circuit = self.ff.External_circuit(self.prob, self._currents, [lambda t: 0.0, lambda t: U_W],
                                                [0.0, float(spec["resistance"])],
                                                [0.0, float(spec.get("capacitance", 0.0))], [0.0, U_W]).bind(self.problem)
        self._timed = [self.circuit]

    def initialise(self):
        return initialise(self.prob)

    def step(self):
        import contextlib, io
        ff = self.ff
        if self._circuit_spec is not None and self.circuit is None:
            self._circuit_setup()
        self.prob.shift_state()                              # :306-307
        self.prob.accept_layers()                            # (dielectric layers: the charge of the step just accepted)
        sink = io.StringIO() if self.quiet else None
        with (contextlib.redirect_stdout(sink) if sink else contextlib.nullcontext()):
            self.t = ff.adaptive_solver(self.solver, self.problem, self.t, self.dt, self.dt_old,
                                        self.u_new, self.u_old, None, None, self.assigner,
                                        self.error, self.error_file, self.max_error, self.ttol,
                                        self.dt_min, time_dependent_arguments=self._timed,
                                        approximation="LFA")
        if self.circuit is not None:
            self.circuit.accept()
        self.newton_iterations += self.prob.last_report.iterations
        self.linear_iterations += self.prob.last_report.linear_iterations
        self.dt_old.time_step = self.dt.time_step            # :335
        self.dt.time_step = ff.adaptive_timestep(self.dt.time_step, self.max_error, self.ttol,
                                                 self.dt_min, self.dt_max)
        self.max_error[2] = self.max_error[1]
        self.max_error[1] = self.max_error[0]
        self.steps += 1
        return self.t

    def diagnose(self):
        """One row of DIAGNOSTIC_COLUMNS from the device-resident state (no download); the set-up is made at the
        first call."""
        if getattr(self, "_diagnose", None) is None:
            self._diagnose = diagnostics(self.prob)
        d = self._diagnose()
        if not d.finite:
            raise RuntimeError("diagnostics: the state is not finite")
        dens = d.density_max
        return dict(zip(DIAGNOSTIC_COLUMNS, (
            self.t, d.z_head, d.window_max, d.field_max, d.species_integral[0], d.species_integral[1], d.net_charge,
            d.surface_charge[0], d.surface_charge[1], d.current, dens[0], dens[1])))

    def surface_charge(self):
        """Per dielectric layer tag the surface charge, the layer's displacement charge [C] and its voltage, of the
        last accepted step (``DeviceProblem.dielectric_charge``; one small read-back).  The time loop leaves the accept
        of a step to the state shift of the next one; a step that is still waiting for it is accepted here first, so
        the figures never lag (the accept depends on ``u_new`` and the step sizes alone: before or behind the shift it
        gives the same charge, and it is made once)."""
        self.prob.accept_layers()
        return self.prob.dielectric_charge(vertices=False)

    def currents(self):
        """The electrode currents of the device-resident state (``fedm_amd.functions.Electrode_currents``; no download):
        electrode 0 the cathode (tag 1), electrode 1 the anode (tag 2), their weighting potentials solved for on the
        device at the first call.  Returns a :class:`fedm_amd.device.Currents`."""
        if getattr(self, "_currents", None) is None:
            self._currents = self.ff.Electrode_currents(self.prob, boundary_tags=(1, 2))
        return self._currents()

    def fields(self, names, t_out=None, t_old=None, probes=None, projection="lumped"):
        """Derived nodal fields of the device-resident state (``fedm_amd.functions.Field_output``; no download): a dict
        name -> nodal array, blended to ``t_out`` between ``t_old`` and the current time when both are given.
        ``probes``: points [n, 2], evaluated as well (``"probes"``).  The set-up is made at the first call and again
        when the names, the points or the projection change."""
        key = (tuple(names), None if probes is None else np.asarray(probes, dtype=np.float64).tobytes(), projection)
        if getattr(self, "_fields_key", None) != key:
            self._fields = self.ff.Field_output(self.prob, list(names), probes=probes, projection=projection,
                                                species_names=SPECIES_NAMES)
            self._fields_key = key
        return self._fields(t_out, t_old, None if t_out is None else self.t)

    def snapshot(self):
        """Checkpoint of the time loop: the three states stay on the device (fedm_state_snapshot), the
        script-level scalars (time, step sizes, error history, counters) are returned -- and, for a problem with
        dielectric layers, the layers' charge and its predecessor, which the device-side snapshot does not cover."""
        self.prob.snapshot_state()
        snap = dict(t=self.t, steps=self.steps, dt=self.dt.time_step, dt_old=self.dt_old.time_step,
                    error=list(self.error), max_error=list(self.max_error),
                    newton=self.newton_iterations, linear=self.linear_iterations)
        if getattr(self.prob.model, "dielectric", None) is not None:
            self.prob.accept_layers()           # (a step still waiting for its accept belongs to the checkpoint)
            charge = self.prob.dielectric_charge()
            snap["layer_charge"] = (charge["q"], charge["q_old"])
        return snap

    def restore(self, snap):
        self.prob.restore_state()
        if "layer_charge" in snap:
            self.prob.set_dielectric_charge(*snap["layer_charge"])
        self.t, self.steps = snap["t"], snap["steps"]
        self.dt.time_step, self.dt_old.time_step = snap["dt"], snap["dt_old"]
        self.error[:], self.max_error[:] = snap["error"], snap["max_error"]
        self.newton_iterations, self.linear_iterations = snap["newton"], snap["linear"]

    def log_rows(self):
        return [tuple(float(v) for v in line.split()) for line in open(self.error_file)]

    def sizes(self):
        return self.prob.sizes()

    def time_kernel(self, kind, repeats):
        return self.prob.time_kernel(kind, repeats)

    def profile(self, enable=True):
        self.prob.profile(enable)

    def profile_read(self):
        return self.prob.profile_read()


def run(prob, T_final=1e-10, max_steps=None, initialise_state=True, **kw):
    """Time loop of fedm-streamer.py:304-340 on the device.  Returns the error-log rows."""
    st = Stepper(prob, **kw)
    if initialise_state:
        st.initialise()
    while abs(st.t - T_final) / T_final > 1e-6:
        st.step()
        if max_steps is not None and st.steps >= max_steps:
            break
    return dict(log=st.log_rows(), t=st.t, steps=st.steps,
                newton_iterations=st.newton_iterations, linear_iterations=st.linear_iterations)
