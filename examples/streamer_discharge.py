#!/usr/bin/env python3
"""Positive streamer in atmospheric air between two planar electrodes (the benchmark of Bagheri et
al., Plasma Sources Sci. Technol. 27 (2018) 095002, case 1) on one MI355X through the fedm_amd facade.

A driver of our own for the functions a FEDM user knows (`fedm.functions`, `fedm.file_io`): the deck
is read with the deck readers, the weak form is put together from `weak_form_balance_equation_log_
representation`, `weak_form_Poisson_equation`, `Flux` and `Boundary_flux`, the time loop is
`adaptive_solver` + `adaptive_timestep`, results go through `file_output`.  It solves the case of
the reference's examples/streamer_discharge/fedm-streamer.py (same deck, boundary table, initial
condition, tolerances and end time), so the two can be compared; that the reference's script itself
lowers to the same device model is checked in tests/test_reference_scripts.py, in the build
container, against the script where it lies.

The mesh is loaded from a DOLFIN XML file like the reference's; as that file is not distributed
(.MISSING_LARGE_BLOBS), `--mesh-spacing` generates a locally refined unstructured stand-in first
(`fedm_amd.cases.streamer.refined_mesh`).  `--cells N` runs on an N x N graded tensor-product mesh
instead (the headline bench's mesh).  `--model tabulated_model` takes the deck whose electron coefficients are
E/N tables (an extension: `fedm.Coefficient_table`, looked up in the element kernels at the cell's own field).
`--photoionization` adds the non-local source of case 3 of the same paper in the three-term Helmholtz approximation
(an extension: `fedm.Photoionization_source`); off by default.
`--diagnostics FILE` writes one row per accepted step (every N-th with `--diagnostics-every N`): head position, field
maximum in the channel, particle numbers, net charge, electrode charges and the induced current, computed on the
device without downloading the state (an extension: `fedm.Discharge_diagnostics`); off by default.
`--ballast OHMS [--stray-capacitance F] [--circuit-log FILE]` runs the anode behind a series resistor with a stray
capacitance to ground, closed on the device (an extension: `fedm.External_circuit`), and writes t, the source's voltage,
the anode's potential, the lead current, e cond and e G per accepted step; off by default.
`--dielectric TAG:THICKNESS[:EPS_R] [--surface-charge-log FILE]` makes the boundary with that tag a dielectric layer
with the electrode's conductor behind it and the surface charge built implicitly on the device (an extension:
`fedm.Dielectric_layer`; 1 coats the cathode, 2 the anode), and writes t, the surface charge, the layer's displacement
charge and its voltage per accepted step; off by default.
`--currents FILE` writes t and the conduction, displacement and total current of the cathode and of the anode per
accepted step (every N-th with `--currents-every N`), with weighting potentials solved for on the device (an extension:
`fedm.Electrode_currents`); off by default.
`--fields LIST` writes derived fields (`E_norm,charge,rate:0,flux_z:1,...`) as VTU series at the output times (every
N-th of them with `--fields-every N`), projected and blended to the output time on the device; `--axis-profile FILE`
writes one row of `E_z` and `n_e` on `r = 0` per accepted step (an extension: `fedm.Field_output`); off by default.

    python examples/streamer_discharge.py --mesh-spacing 8e-6 --end 1.4e-8 --out streamer_output
"""
import argparse
import contextlib
import io
import sys
from dataclasses import dataclass, field
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fedm_amd import forms as fem                          # noqa: E402  (what `dolfin` is to a FEDM script)
from fedm_amd import file_io, functions as fedm            # noqa: E402
from fedm_amd.physical_constants import elementary_charge, epsilon_0     # noqa: E402
from fedm_amd.termsum import parse as deck_expression      # noqa: E402

REPO = Path(__file__).resolve().parent.parent
# Photoionisation (Bagheri et al. 2018, case 3): the three-term Helmholtz fit of Bourdon et al. 2007 for air and the
# case's efficiency.  QUOTED FROM MEMORY -- the papers were not at hand when this was written; check them before
# relying on a run.  No test depends on these numbers.
PHOTO_A = (1.986e-4, 0.0051, 0.4886)            # [1/(cm^2 Torr^2)]
PHOTO_LAMBDA = (0.0553, 0.1460, 0.89)           # [1/(cm Torr)]
PHOTO_P_O2 = 150.0                              # partial pressure of oxygen [Torr]
PHOTO_EFFICIENCY = 0.075 * 30.0 / (750.0 + 30.0)    # xi * p_q / (p + p_q)
CHANNEL_RADIUS = 0.9e-3        # cells nearer to the axis than this mark the streamer's head (the mesh's finest region)
DIAGNOSTICS_COLUMNS = ("t", "z_head", "E_max", "N_e", "N_i", "net_charge", "surface_charge_cathode",
                       "surface_charge_anode", "current")
AXIS_POINTS = 64               # points of --axis-profile on r = 0, from the cathode to the anode
SEED = "std::log(1e13+5e18*exp(-(pow(x[0], 2)+pow(x[1]-1e-2, 2))/pow(0.4e-3, 2)))"    # ions: background + seed
BACKGROUND = "std::log(1e13)"                                                           # electrons


@dataclass
class Case:
    """Conditions of the run (Bagheri et al. 2018, case 1; values as in fedm-streamer.py:26-41,67-76,96-108)."""
    deck: str = "benchmark_model"
    pressure_torr: float = 760.0
    gas_temperature: float = 300.0
    anode_voltage: float = 18750.0
    side: float = 0.0125                        # the domain is side x side in (r, z)
    end_time: float = 1.4e-8
    first_step: float = 5e-12
    longest_step: float = 5e-12
    shortest_step: float = 1e-15
    step_tolerance: float = 1e-3
    newton_rtol: float = 1e-4
    newton_max_it: int = 20
    kinds: tuple = ("reaction", "drift-diffusion-reaction")        # ions do not move, electrons drift and diffuse
    roles: tuple = ("Ions", "electrons")
    output_windows: tuple = (1e-11, 1e-10, 1e-9)
    # per boundary (cathode z=0, anode z=side, axis r=0, outer wall r=side): condition per species
    walls: dict = field(default_factory=lambda: {
        "cathode": ("zero flux", "Neumann"), "anode": ("zero flux", "Neumann"),
        "axis": ("zero flux", "zero flux"), "outer": ("zero flux", "zero flux")})

    @property
    def gas_density(self):
        return self.pressure_torr * 3.21877e22

    def wall_lines(self):
        s = self.side
        return {"cathode": ["line", 0.0, 0.0, 0.0, s], "anode": ["line", s, s, 0.0, s],
                "axis": ["line", 0.0, s, 0.0, 0.0], "outer": ["line", 0.0, s, s, s]}


def read_deck(case, input_dir):
    """Species, charges and transport data through the FEDM deck readers."""
    file_io.files.file_input = Path(input_dir) if input_dir else REPO / "decks" / "streamer_discharge" / "file_input"
    deck_dir = file_io.files.file_input / case.deck
    n_species, names, property_files, file_names = file_io.read_speclist(deck_dir)
    masses, charge_numbers = file_io.read_particle_properties(property_files, case.deck)
    n_species, n_equations, names, masses, charge_numbers = fedm.modify_approximation_vars(
        "LFA", n_species, names, masses, charge_numbers)
    diffusion_x, diffusion, diffusion_dep = file_io.read_transport_coefficients(names, "Diffusion", case.deck)
    mobility_x, mobility, mobility_dep = file_io.read_transport_coefficients(names, "mobility", case.deck)
    # the ionisation coefficient: the benchmark deck's closed form is written out in coupled_form like in the
    # reference's script; a deck may give alpha / N against E/N instead
    alpha_file = deck_dir / "transport_coefficients" / "alpha.dat"
    ionisation = None
    if file_io.read_dependence(alpha_file) == "E/N":
        (alpha_x,), (alpha_y,) = file_io.read_rate_coefficients([alpha_file], ["E/N"])
        ionisation = (alpha_x, alpha_y)
    return dict(n_species=n_species, n_equations=n_equations, names=names, file_names=file_names, masses=masses,
                charge_numbers=charge_numbers, diffusion=diffusion, mobility=mobility,
                diffusion_x=diffusion_x, mobility_x=mobility_x, diffusion_dep=diffusion_dep, mobility_dep=mobility_dep,
                ionisation=ionisation)


def load_mesh(case, cells, mesh_spacing, mesh_file, workdir):
    if cells:
        from fedm_amd.mesh import geometric_lines
        return fem.RectangleMesh((0.0, 0.0), (case.side, case.side), cells, cells,
                                 x_lines=geometric_lines(case.side, cells, 4.0))
    if mesh_file is None:
        from fedm_amd.cases import streamer
        from fedm_amd import mesh_io
        mesh_file = Path(workdir) / "mesh.xml"
        mesh_file.parent.mkdir(parents=True, exist_ok=True)
        mesh_io.write_dolfin_xml(streamer.refined_mesh(mesh_spacing), mesh_file)
    return fem.Mesh(str(mesh_file))


class Fields:
    """The mixed space of the coupled system, the scalar space of its parts, and the Functions."""

    def __init__(self, mesh, n_equations):
        lagrange = fem.FiniteElement("Lagrange", mesh.ufl_cell(), 1)
        self.mixed = fem.FunctionSpace(mesh, fem.MixedElement(fedm.Mixed_element_list(n_equations, lagrange)))
        self.scalar = fem.FunctionSpace(mesh, lagrange)
        parts = fedm.Function_space_list(n_equations, self.scalar)
        self.split = fem.FunctionAssigner(parts, self.mixed)          # mixed -> parts
        self.join = fem.FunctionAssigner(self.mixed, parts)           # parts -> mixed
        self.trial, self.tests = fem.TrialFunction(self.mixed), fem.TestFunctions(self.mixed)
        self.now, self.before, self.before2 = (fem.Function(self.mixed) for _ in range(3))
        self.parts_now = fedm.Function_definition(self.scalar, "Function", n_equations)
        self.parts_before = fedm.Function_definition(self.scalar, "Function", n_equations)
        self.scratch = fem.Function(self.scalar)


def electrode_conditions(case, space, coated=None):
    """Dirichlet values of the potential on the two electrodes for `space` (scalar or a sub-space); `coated`: the tag
    of an electrode behind a dielectric layer (1: the cathode, 2: the anode), which gets none -- the conductor is behind
    the layer, and the layer's own condition stands on that boundary."""
    def on_cathode(x, on_boundary):
        return on_boundary and fem.near(x[1], 0)

    def on_anode(x, on_boundary):
        return on_boundary and fem.near(x[1], case.side)
    conditions = {1: fem.DirichletBC(space, fem.Constant(0.0), on_cathode),
                  2: fem.DirichletBC(space, fem.Constant(case.anode_voltage), on_anode)}
    return [bc for tag, bc in conditions.items() if tag != coated]


def parse_dielectric(text):
    """`TAG:THICKNESS[:EPS_R]` -> (tag, thickness [m], eps_r); eps_r = 1 where it is not given"""
    parts = str(text).split(":")
    if len(parts) not in (2, 3):
        raise ValueError(f"--dielectric {text!r}: expected TAG:THICKNESS[:EPS_R]")
    return int(parts[0]), float(parts[1]), float(parts[2]) if len(parts) == 3 else 1.0


def initial_state(case, deck, fl, dx, radius, writers, t):
    """Seed + background densities and the potential they produce (one linear Poisson solve)."""
    for k, text in enumerate((SEED, BACKGROUND)):
        for target in (fl.parts_before, fl.parts_now):
            target[k] = fem.interpolate(fem.Expression(text, degree=1), fl.scalar)
    for k, writer in enumerate(writers["density"]):
        fl.scratch.assign(fl.parts_before[k])
        fl.scratch.rename(deck["file_names"][k + 1], str(k + 1))
        writer << (fl.scratch, t)
    space_charge = (fem.exp(fl.parts_before[0]) - fem.exp(fl.parts_before[1])) * elementary_charge / epsilon_0
    poisson = fedm.weak_form_Poisson_equation(dx, fem.TrialFunction(fl.scalar), fem.TestFunction(fl.scalar),
                                              space_charge, radius)
    conditions = electrode_conditions(case, fl.scalar)
    matrix, load = fem.assemble(fem.lhs(poisson)), fem.assemble(fem.rhs(poisson))
    for condition in conditions:
        condition.apply(matrix)
        condition.apply(load)
    potential = fem.Function(fl.scalar)
    fem.solve(matrix, potential.vector(), load)
    fl.scratch.assign(potential)
    writers["potential"] << (fl.scratch, t)
    for target in (fl.parts_before, fl.parts_now):
        target[-1].assign(potential)


def coupled_form(case, deck, fl, mesh, dx, radius, dt, dt_before, photoionization=False, dielectric=None):
    """Ion and electron balance in logarithmic variables + Poisson, local field approximation.  `dielectric`: (tag,
    thickness, eps_r) of a boundary that is a dielectric layer; the conductor behind it has the voltage of the electrode
    the layer coats (0 V on any other boundary)."""
    wall_tags = fedm.Marking_boundaries(mesh, list(case.wall_lines().values()))
    ds = fem.Measure("ds", domain=mesh, subdomain_data=wall_tags)
    outward = fem.FacetNormal(mesh)
    u, v = fl.trial, fl.tests
    n_sp, i_phi = deck["n_species"], deck["n_equations"] - 1
    field_vector = -fem.grad(u[i_phi])
    field_strength = fem.sqrt(fem.inner(-fem.grad(u[i_phi]), -fem.grad(u[i_phi])))
    # the deck gives the electron coefficients as expressions of the field strength E_m (parsed, not
    # eval'd) or as tables of N * coefficient against E/N (looked up at the cell's own field, implicitly);
    # the ions of this model do not move
    def electron_coefficient(what):
        if deck[what + "_dep"][1] == "E/N":
            return fedm.Coefficient_table(field_strength, deck[what + "_x"][1], deck[what][1],
                                          case.gas_density) / case.gas_density
        return deck_expression(deck[what][1])
    mobility = [deck["mobility"][0], electron_coefficient("mobility")]
    diffusion = [deck["diffusion"][0], electron_coefficient("diffusion")]
    if deck["ionisation"] is not None:
        ionisation = fedm.Coefficient_table(field_strength, *deck["ionisation"], case.gas_density) * case.gas_density
    else:
        ionisation = (1.1944e6 + 4.3666e26 * field_strength ** (-3)) * fem.exp(-2.73e7 / field_strength) - 340.75
    production = ionisation * mobility[1] * field_strength * fem.exp(u[1])            # alpha |mu E| n_e
    sources = [production, production]
    if photoionization:
        # every photo-electron leaves an ion behind: both balances receive the source; the Helmholtz solutions
        # vanish on the two electrodes (tags 1 and 2), zero flux on the axis and the outer wall
        photo = fedm.Photoionization_source(production, PHOTO_EFFICIENCY, PHOTO_A, PHOTO_LAMBDA, PHOTO_P_O2,
                                            zero_on=[ds(1), ds(2)])
        sources = [production + photo, production + photo]
    fluxes = [0.0, fedm.Flux(deck["charge_numbers"][1], u[1], diffusion[1], mobility[1], field_vector,
                             grad_diffusion=False)]
    charge_density = sum(z * fem.exp(u[k]) * elementary_charge / epsilon_0
                         for k, z in enumerate(deck["charge_numbers"][:n_sp]))
    form = 0.0
    for k in range(n_sp):
        form += fedm.weak_form_balance_equation_log_representation(
            case.kinds[k], dt, dt_before, dx, u[k], fl.before[k], fl.before2[k], v[k], sources[k], fluxes[k],
            radius, diffusion[k])
    form += fedm.weak_form_Poisson_equation(dx, u[i_phi], v[i_phi], charge_density, radius)
    for tag, wall in enumerate(case.walls, start=1):
        for k in range(n_sp):
            form += fedm.Boundary_flux(case.walls[wall][k], case.kinds[k], case.roles[k], deck["charge_numbers"][k],
                                       mobility[k], field_vector, outward, u[k], 0.0, v[k], ds(tag), radius)
    if dielectric is not None:
        tag, thickness, eps_r = dielectric
        form += fedm.Dielectric_layer(u[i_phi], v[i_phi], ds(tag), thickness, eps_r,
                                      voltage={1: 0.0, 2: case.anode_voltage}.get(tag, 0.0), r=radius)
    return form, wall_tags


def quiet_stdout(quiet):
    return contextlib.redirect_stdout(io.StringIO()) if quiet else contextlib.nullcontext()


CURRENTS_COLUMNS = ("t", "conduction_cathode", "displacement_cathode", "total_cathode", "conduction_anode",
                    "displacement_anode", "total_anode")


def currents_row(t, c):
    """One `--currents` row from a `fedm_amd.device.Currents`: t, then conduction, displacement and total [A] per electrode."""
    return [t] + [x for g in range(len(c.conduction)) for x in (c.conduction[g], c.displacement[g], c.total[g])]


CIRCUIT_COLUMNS = ("t", "V_s", "U", "lead_current", "conduction", "conductance")
SURFACE_CHARGE_COLUMNS = ("t", "surface_charge", "displacement_charge", "voltage")


def main(cells=None, mesh_spacing=2.5e-5, mesh_file=None, end_time=None, input_dir=None, output_dir=None,
         quiet=False, stop_before_device=None, coupling="coupled", model="benchmark_model", photoionization=False,
         diagnostics=None, diagnostics_every=1, fields=None, fields_every=1, axis_profile=None, currents=None,
         currents_every=1, ballast=None, stray_capacitance=0.0, circuit_log=None, dielectric=None,
         surface_charge_log=None):
    """Runs the case; returns (state as (n_vertices, 3) array of ln n_i, ln n_e, Phi; error-log path).
    `model`: the deck folder under the input directory ("benchmark_model", "tabulated_model").
    `photoionization`: add the Helmholtz photoionisation source (coupled step only).
    `diagnostics`: a file that receives DIAGNOSTICS_COLUMNS per accepted step (every `diagnostics_every`-th).
    `fields`: names of derived fields (fedm.Field_output) written as VTU series under `<output>/fields/` at the output
    times (every `fields_every`-th of them).  `axis_profile`: a file that receives, per accepted step, t followed by
    E_z and then n_e at the AXIS_POINTS points of the axis (the first row holds their z).  `currents`: a file that
    receives, per accepted step (every `currents_every`-th), t and then conduction, displacement and total current [A] of
    the cathode and of the anode (fedm.Electrode_currents, their weighting potentials solved for on the device).
    `ballast`: a series resistance [ohm] between the source and the anode, with `stray_capacitance` [F] to ground in
    parallel (fedm.External_circuit; the cathode stays an ideal ground); `circuit_log`: a file that receives
    CIRCUIT_COLUMNS of the anode per accepted step.
    `dielectric`: `TAG:THICKNESS[:EPS_R]`, the boundary with that tag becomes a dielectric layer (fedm.Dielectric_layer:
    tag 1 coats the cathode, tag 2 the anode, whose Dirichlet values leave; coupled step only; the initial potential is
    that of the bare electrodes); `surface_charge_log`: a file that receives SURFACE_CHARGE_COLUMNS per accepted step.
    None: the path as it was."""
    layer = parse_dielectric(dielectric) if dielectric is not None else None
    if layer is not None and coupling != "coupled":
        raise ValueError("--dielectric runs with the coupled step only")
    if surface_charge_log is not None and layer is None:
        raise ValueError("--surface-charge-log needs --dielectric")
    case = Case(deck=model) if end_time is None else Case(deck=model, end_time=end_time)
    fem.parameters["form_compiler"]["quadrature_degree"] = 2
    deck = read_deck(case, input_dir)
    if output_dir is not None:
        file_io.files.output_folder_path = Path(output_dir)
    out = file_io.files.output_folder_path
    writers = {"density": file_io.output_files("pvd", "number density", list(case.roles)),
               "potential": file_io.output_files("pvd", "potential", ["Phi"])[0]}
    dt = fem.Expression("time_step", time_step=case.first_step, degree=0)
    dt_before = fem.Expression("time_step", time_step=1e30, degree=0)     # "no previous step": BDF2 starts as BDF1
    charges = [z * elementary_charge for z in deck["charge_numbers"]]
    file_io.log("conditions", file_io.files.model_log, dt.time_step, case.anode_voltage, case.pressure_torr, case.side,
                case.gas_density, case.gas_temperature)
    file_io.log("properties", file_io.files.model_log, "Air", case.deck, deck["file_names"], deck["masses"], charges)

    mesh = load_mesh(case, cells, mesh_spacing, mesh_file, out / "mesh")
    with quiet_stdout(quiet):
        file_io.mesh_statistics(mesh)
    radius = fem.Expression("x[0]", degree=1)
    dx = fem.Measure("dx", domain=mesh)
    fl = Fields(mesh, deck["n_equations"])
    t = 0.0
    file_io.log("initial time", file_io.files.model_log, t)
    initial_state(case, deck, fl, dx, radius, writers, t)
    form, wall_tags = coupled_form(case, deck, fl, mesh, dx, radius, dt, dt_before, photoionization, layer)
    fem.File(str(out / "mesh" / "boundary_mesh_function.pvd")) << wall_tags
    fl.join.assign(fl.before, list(fl.parts_before))
    fl.join.assign(fl.now, list(fl.parts_now))

    residual = fem.action(form, fl.now)
    jacobian = fem.derivative(residual, fl.now, fl.trial)
    build_problem = stop_before_device or fedm.Problem
    problem = build_problem(jacobian, residual, electrode_conditions(case, fl.mixed.sub(deck["n_equations"] - 1),
                                                                     coated=layer[0] if layer is not None else None))
    problem.device.setup_multigrid(nu=1)                 # preconditioner of the device's GMRES (no script counterpart)
    diagnose = rows = None
    if diagnostics is not None:
        # electrodes: tags 1 (cathode) and 2 (anode) of wall_lines(); psi = z / gap is exact for the planar gap
        diagnose = fedm.Discharge_diagnostics(problem, boundary_tags=(1, 2),
                                              window=(0.0, CHANNEL_RADIUS, 0.0, case.side),
                                              weighting_potential=mesh.coords[:, 1] / case.side)
        rows = open(diagnostics, "w")
        rows.write("# " + " ".join(DIAGNOSTICS_COLUMNS) + "\n")
    currents_of = current_rows = None
    if currents is not None:
        currents_of = fedm.Electrode_currents(problem, boundary_tags=(1, 2))
        current_rows = open(currents, "w")
        current_rows.write("# " + " ".join(CURRENTS_COLUMNS) + "\n")
    charge_rows = None
    if surface_charge_log is not None:
        charge_rows = open(surface_charge_log, "w")
        charge_rows.write("# " + " ".join(SURFACE_CHARGE_COLUMNS) + "\n")
    circuit = circuit_rows = None
    timed = []
    if ballast is not None:
        # the anode (tag 2) behind the resistor, starting at the source's voltage; the cathode (tag 1) an ideal ground
        electrodes = currents_of or fedm.Electrode_currents(problem, boundary_tags=(1, 2))
        circuit = fedm.External_circuit(problem, electrodes, [lambda s: 0.0, lambda s: case.anode_voltage],
                                        [0.0, float(ballast)], [0.0, float(stray_capacitance)],
                                        [0.0, case.anode_voltage]).bind(problem)
        timed = [circuit]
        if circuit_log is not None:
            circuit_rows = open(circuit_log, "w")
            circuit_rows.write("# " + " ".join(CIRCUIT_COLUMNS) + "\n")
    field_out = field_files = profile = profile_rows = None
    if fields:
        fields = [name.strip() for name in (fields.split(",") if isinstance(fields, str) else fields) if name.strip()]
        field_out = fedm.Field_output(problem, fields, species_names=[r.lower() for r in case.roles])
        field_files = file_io.output_files("pvd", "fields", [name.replace(":", "_") for name in fields])
        for writer in field_files:
            writer.mesh = mesh
    if axis_profile is not None:
        # its own set-up on the same problem: fedm_fields takes the requests per call, the points belong to the context
        import numpy as np
        z_axis = np.linspace(0.0, case.side, AXIS_POINTS)
        profile = fedm.Field_output(problem, ["E_z", "density:electrons"], probes=np.column_stack([0.0 * z_axis, z_axis]),
                                    species_names=[r.lower() for r in case.roles])
        profile_rows = open(axis_profile, "w")
        profile_rows.write("# t, E_z[%d], n_e[%d] on r = 0; first row: nan and the points' z twice\n" % (AXIS_POINTS, AXIS_POINTS))
        profile_rows.write(" ".join(f"{x:.17g}" for x in [float("nan"), *z_axis, *z_axis]) + "\n")
    accepted = outputs = 0
    newton = fedm.PETScSNESSolver()
    newton.parameters["relative_tolerance"] = case.newton_rtol
    newton.parameters["maximum_iterations"] = case.newton_max_it
    newton.parameters["linear_solver"] = "gmres"
    newton.parameters["coupling"] = coupling             # "uncoupled": Poisson solve, then Newton on the species alone

    # what file_output interpolates between: potential first, then the species
    order = [deck["n_equations"] - 1] + list(range(deck["n_species"]))
    out_files = [writers["potential"]] + list(writers["density"])
    out_names = ["Phi"] + list(case.roles)
    out_now, out_before = [fl.parts_now[k] for k in order], [fl.parts_before[k] for k in order]
    window, stride = case.output_windows[0], case.output_windows[0]
    step_errors, recent_errors = [0.0] * deck["n_species"], [1] * 3
    while abs(t - case.end_time) / case.end_time > 1e-6:
        t_before = t
        fl.before2.assign(fl.before)
        fl.before.assign(fl.now)
        fl.split.assign(list(fl.parts_before), fl.before)
        with quiet_stdout(quiet):
            t = fedm.adaptive_solver(newton, problem, t, dt, dt_before, fl.now, fl.before, list(fl.parts_now),
                                     list(fl.parts_before), fl.split, step_errors, file_io.files.error_file,
                                     recent_errors, case.step_tolerance, case.shortest_step,
                                     time_dependent_arguments=timed, approximation="LFA")
        file_io.log("time", file_io.files.model_log, t)
        if circuit is not None:     # the accepted step: the history moves on, conduction and conductance of the new state
            circuit.accept()
            if circuit_rows is not None:
                circuit_rows.write(" ".join(f"{x:.17g}" for x in circuit.log_row(t, 1)) + "\n")
                circuit_rows.flush()
        if charge_rows is not None:
            # (the accept of this step, which the next state shift would make: made here, once, so the row does not lag)
            problem.device.accept_layers()
            charge = problem.device.dielectric_charge(vertices=False)
            charge_rows.write(" ".join(f"{x:.17g}" for x in (t, charge["charge"][layer[0]], charge["displacement"][layer[0]],
                                                              charge["voltage"][layer[0]])) + "\n")
            charge_rows.flush()
        dt_before.time_step = dt.time_step
        dt.time_step = fedm.adaptive_timestep(dt.time_step, recent_errors, case.step_tolerance, case.shortest_step,
                                              case.longest_step)
        recent_errors[1:] = recent_errors[:2]
        accepted += 1
        if diagnose is not None and accepted % max(1, int(diagnostics_every)) == 0:
            d = diagnose()
            row = (t, d.z_head, d.window_max, d.species_integral[1], d.species_integral[0], d.net_charge,
                   d.surface_charge[0], d.surface_charge[1], d.current)
            rows.write(" ".join(f"{x:.17g}" for x in row) + "\n")
            rows.flush()
        if currents_of is not None and accepted % max(1, int(currents_every)) == 0:
            current_rows.write(" ".join(f"{x:.17g}" for x in currents_row(t, currents_of())) + "\n")
            current_rows.flush()
        if profile is not None:
            p = profile()["probes"]
            profile_rows.write(" ".join(f"{x:.17g}" for x in [t, *p[0], *p[1]]) + "\n")
            profile_rows.flush()
        if field_out is not None:
            from fedm_amd.mesh_io import output_times
            for t_out in output_times(t, window, stride, list(case.output_windows), list(case.output_windows))[0]:
                outputs += 1
                if outputs % max(1, int(fields_every)):
                    continue
                values = field_out(t_out, t_before, t)
                for name, writer in zip(fields, field_files):
                    writer.write(values[name], name, t_out)
        window, stride = file_io.file_output(t, t_before, window, stride, list(case.output_windows),
                                             list(case.output_windows), ["pvd"] * len(order), out_files, out_names,
                                             out_now, out_before)
    if rows is not None:
        rows.close()
    if profile_rows is not None:
        profile_rows.close()
    if current_rows is not None:
        current_rows.close()
    if circuit_rows is not None:
        circuit_rows.close()
    if charge_rows is not None:
        charge_rows.close()
    return problem.device.get_state(), file_io.files.error_file


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cells", type=int, help="N x N graded tensor-product mesh instead of the unstructured one")
    ap.add_argument("--mesh-spacing", type=float, default=2.5e-5, help="finest spacing of the generated mesh [m]")
    ap.add_argument("--mesh", help="DOLFIN XML mesh to load instead of generating one")
    ap.add_argument("--end", type=float, default=1e-10, help="end time [s] (the reference script: 1.4e-8)")
    ap.add_argument("--out", default="streamer_output")
    ap.add_argument("--coupling", choices=["coupled", "uncoupled"], default="coupled",
                    help="one Newton solve on the mixed space, or the segregated step")
    ap.add_argument("--model", default="benchmark_model",
                    help="deck folder: benchmark_model (closed-form coefficients) or tabulated_model (E/N tables)")
    ap.add_argument("--photoionization", action="store_true",
                    help="add the three-term Helmholtz photoionisation source (coefficients quoted from memory, see the source)")
    ap.add_argument("--diagnostics", metavar="FILE",
                    help="write t, z_head, E_max, N_e, N_i, net charge, electrode charges and current per accepted step")
    ap.add_argument("--diagnostics-every", type=int, default=1, metavar="N", help="... every N-th accepted step")
    ap.add_argument("--fields", metavar="LIST",
                    help="comma-separated derived fields written at the output times: E_norm, E_r, E_z, charge, "
                         "density:electrons, rate:0, flux_r:1, flux_z:1, state:2")
    ap.add_argument("--fields-every", type=int, default=1, metavar="N", help="... at every N-th output time")
    ap.add_argument("--axis-profile", metavar="FILE", help="write E_z and n_e on r = 0 per accepted step")
    ap.add_argument("--currents", metavar="FILE",
                    help="write t and the conduction, displacement and total current of cathode and anode per accepted step")
    ap.add_argument("--currents-every", type=int, default=1, metavar="N", help="... every N-th accepted step")
    ap.add_argument("--ballast", type=float, metavar="OHMS",
                    help="run the anode behind a series resistor (fedm.External_circuit); off by default")
    ap.add_argument("--stray-capacitance", type=float, default=0.0, metavar="F", help="... with this capacitance to ground in parallel")
    ap.add_argument("--circuit-log", metavar="FILE",
                    help="... and write %s of the anode per accepted step" % ", ".join(CIRCUIT_COLUMNS))
    ap.add_argument("--dielectric", metavar="TAG:THICKNESS[:EPS_R]",
                    help="make the boundary with that tag a dielectric layer (fedm.Dielectric_layer; 1: the cathode, 2: the "
                         "anode); off by default")
    ap.add_argument("--surface-charge-log", metavar="FILE",
                    help="... and write %s of the layer per accepted step" % ", ".join(SURFACE_CHARGE_COLUMNS))
    ap.add_argument("--save-state", metavar="FILE", help="write the final state (n_vertices, 3) as a .npy file")
    a = ap.parse_args()
    state, log_path = main(cells=a.cells, mesh_spacing=a.mesh_spacing, mesh_file=a.mesh, end_time=a.end,
                           output_dir=a.out, coupling=a.coupling, model=a.model, photoionization=a.photoionization,
                           diagnostics=a.diagnostics, diagnostics_every=a.diagnostics_every, fields=a.fields,
                           fields_every=a.fields_every, axis_profile=a.axis_profile, currents=a.currents,
                           currents_every=a.currents_every, ballast=a.ballast, stray_capacitance=a.stray_capacitance,
                           circuit_log=a.circuit_log, dielectric=a.dielectric, surface_charge_log=a.surface_charge_log)
    if a.save_state:
        import numpy
        numpy.save(a.save_state, state)
    print(open(log_path).read())
