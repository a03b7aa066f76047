#!/usr/bin/env python3
"""Abnormal glow discharge in argon at 1 Torr between plane electrodes 1 cm apart: electron energy
balance + Ar*, Ar+ and electron balances + Poisson, local mean energy approximation (LMEA), with
tabulated transport and rate coefficients and a reaction scheme read from the FEDM deck.

A driver of our own for the fedm_amd facade.  It solves the case of the reference's
examples/glow_discharge/fedm-gd.py (deck `4_particles`, 100 x 100 crossed mesh, -250 V switched on
with a 1 ns rise, reflecting metallic electrodes with secondary emission), and the run reproduces
the reference's golden error log and species snapshots (tests/test_gpu_glow_discharge.py).  That the
reference's own script lowers to the same device model is checked in tests/test_reference_scripts.py
in the build container.

The nodal coefficients are refreshed once per time step on the host with
`Transport_coefficient_interpolation` / `Rate_coefficient_interpolation` (as a FEDM script does); the
Newton solves run on the device.  `fedm_amd.cases.glow_discharge.Case` is the variant that keeps the
whole per-step pipeline on the GPU.

    python examples/glow_discharge.py gd_output

`--balance FILE` writes one row per accepted step (every N-th with `--balance-every N`): time, the contents, the
conduction currents into the two electrodes, Joule power, collision loss, the imbalances of the energy and particle
balances and the Shockley-Ramo current with psi = z / gap, all formed on the device without downloading the state (an
extension: `fedm.Discharge_balance`); off by default.
`--ballast OHMS [--stray-capacitance F] [--circuit-log FILE]` runs the powered electrode behind a series resistor with a
stray capacitance to ground, closed on the device (an extension: `fedm.External_circuit`), and writes t, the source's
voltage, the electrode's potential, the lead current, e cond and e G per accepted step; off by default.
`--currents FILE` writes t and the conduction, displacement and total current of the powered and of the grounded
electrode per accepted step (every N-th with `--currents-every N`): the Shockley-Ramo currents with weighting potentials
solved for on the device, the displacement part that of the rising voltage (an extension: `fedm.Electrode_currents`);
off by default.

`--fields LIST` writes derived fields (`mean_energy,E_norm,source:electrons,joule,flux_z:Ar_plus,...`) as VTU series at
the output times (every N-th of them with `--fields-every N`); `--axis-profile FILE` writes, per accepted step, the
profiles of AXIS_FIELDS along r = 0.  Both are formed on the device from the resident state and the coefficient table,
where the residual of the step just solved evaluates them (an extension: `fedm.Field_output`): the values are those of
the accepted step that reaches the output time, at its own time, not blended; off by default.
"""
import argparse
import contextlib
import io
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fedm_amd import forms as fem                          # noqa: E402  (what `dolfin` is to a FEDM script)
from fedm_amd import file_io, functions as fedm            # noqa: E402
from fedm_amd.physical_constants import elementary_charge, epsilon_0, kB     # noqa: E402

REPO = Path(__file__).resolve().parent.parent
DECK = "4_particles"
GAP = RADIUS = 0.01                       # electrode distance and discharge radius [m]
PRESSURE, GAS_TEMPERATURE, VOLTAGE = 1.0, 300.0, -250.0
GAS_DENSITY = PRESSURE * 3.21877e22
# the four sides in the order of the boundary tags: powered electrode (z = 0), grounded electrode
# (z = gap), axis, dielectric outer wall
SIDES = [["line", 0.0, 0.0, 0.0, RADIUS], ["line", GAP, GAP, 0.0, RADIUS],
         ["line", 0.0, GAP, 0.0, 0.0], ["line", 0.0, GAP, RADIUS, RADIUS]]
METAL, OPEN = [0.3, 0.3, 5e-4, 0.3], [1.0, 1.0, 1.0, 1.0]     # reflection coefficients per species
REFLECTION = [METAL, METAL, OPEN, OPEN]
SECONDARY_EMISSION = [0.06, 0.06, 0, 0]
SECONDARY_ENERGY = 5.0                    # mean energy of the emitted electrons [eV]
KINDS = ["reaction", "diffusion-reaction", "drift-diffusion-reaction", "drift-diffusion-reaction"]
WALL_ROLE = ["Heavy", "Heavy", "Heavy", "electrons"]
CHARGE_ROLE = ["Neutral", "Neutral", "Ion", "electrons"]
START_DENSITY = [GAS_DENSITY, 1e12, 1e12, 1e12]
OUTPUT_WINDOWS = [1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5]
OUTPUT_STRIDES = [1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-6]
AXIS_POINTS = 64                          # points of --axis-profile on r = 0, from the powered to the grounded electrode
AXIS_FIELDS = ["mean_energy", "E_z", "density:electrons", "joule"]


def read_deck(input_dir):
    """Species, reaction scheme and coefficient tables; derivatives of the energy-dependent tables
    (needed by the semi-implicit treatment) by finite differences of the tables."""
    file_io.files.file_input = Path(input_dir) if input_dir else REPO / "decks" / "glow_discharge" / "file_input"
    deck_dir = file_io.files.file_input / DECK
    d = {}
    n, d["names"], property_files, d["file_names"] = file_io.read_speclist(deck_dir)
    d["masses"], d["charge_numbers"] = file_io.read_particle_properties(property_files, DECK)
    d["power"], d["loss"], d["gain"] = file_io.reaction_matrices(deck_dir, d["names"])
    rate_files = file_io.rate_coefficient_file_names(deck_dir)
    d["energy_loss"] = file_io.read_energy_loss(deck_dir)
    d["mu_x"], d["mu_y"], d["mu_dep"] = file_io.read_transport_coefficients(d["file_names"], "mobility", DECK)
    d["D_x"], d["D_y"], d["D_dep"] = file_io.read_transport_coefficients(d["file_names"], "Diffusion", DECK)
    d["k_dep"] = file_io.read_dependences(rate_files)
    d["k_x"], d["k_y"] = file_io.read_rate_coefficients(rate_files, d["k_dep"])
    e = n - 1                                                  # the electrons are the last species
    d["dD_e"] = np.gradient(d["D_y"][e], d["D_x"][e]) / GAS_DENSITY
    d["dmu_e"] = np.gradient(d["mu_y"][e], d["mu_x"][e]) / GAS_DENSITY
    d["dk"] = [np.gradient(ky, kx) if dep == "Umean" else 0.0 for kx, ky, dep in zip(d["k_x"], d["k_y"], d["k_dep"])]
    d["n_species"], d["n_equations"], d["names"], d["masses"], d["charge_numbers"] = fedm.modify_approximation_vars(
        "LMEA", n, d["names"], d["masses"], d["charge_numbers"])
    d["n_reactions"] = len(rate_files)
    return d


def reduced_field(potential):
    """|E|/N in Td as a nodal field: the argument of the field-dependent tables."""
    strength = fem.sqrt(fem.dot(-fem.grad(potential), -fem.grad(potential)))
    return fem.project(1e21 * strength / GAS_DENSITY, solver_type="mumps")


class Discharge:
    """Spaces, Functions and nodal coefficient fields of the model."""

    def __init__(self, mesh, deck):
        ns, neq, nr = deck["n_species"], deck["n_equations"], deck["n_reactions"]
        lagrange = fem.FiniteElement("Lagrange", mesh.ufl_cell(), 1)
        self.mixed = fem.FunctionSpace(mesh, fem.MixedElement(fedm.Mixed_element_list(neq, lagrange)))
        self.scalar = V = fem.FunctionSpace(mesh, lagrange)
        parts = fedm.Function_space_list(neq, V)
        self.split, self.join = fem.FunctionAssigner(parts, self.mixed), fem.FunctionAssigner(self.mixed, parts)
        self.trial, self.tests = fem.TrialFunction(self.mixed), fem.TestFunctions(self.mixed)
        self.now, self.before, self.before2 = (fem.Function(self.mixed) for _ in range(3))
        self.phi, self.phi_before, self.phi_before2 = (fem.Function(V) for _ in range(3))
        self.field, self.field_before = fem.Function(V), fem.Function(V)
        self.dens_now, self.dens_before, self.dens_before2 = (fedm.Function_definition(V, "Function", ns) for _ in range(3))
        self.energy, self.energy_before, self.energy_before2 = (fem.Function(V) for _ in range(3))
        self.D, self.dD, self.mu, self.dmu = (fedm.Function_definition(V, "Function", ns) for _ in range(4))
        self.k, self.dk = (fedm.Function_definition(V, "Function", nr) for _ in range(2))
        self.scratch = fem.Function(V)

    def start(self, deck, writers, t):
        """Uniform start: 3 eV mean energy, 1e12 m^-3 of every charged or excited species."""
        V, e = self.scalar, deck["n_species"] - 1
        three_ev = fem.interpolate(fem.Expression("3.0", degree=1), V)
        self.energy.assign(three_ev)
        self.energy_before.assign(three_ev)
        self.energy_before2.assign(fem.Constant(0.0))
        for k, n0 in enumerate(START_DENSITY):
            ln_n = fem.Expression("std::log(ic)", ic=n0, degree=1)
            self.dens_now[k].assign(ln_n)
            self.dens_before[k].assign(ln_n)
            self.dens_before2[k].assign(fem.Constant(0.0))
        # the energy equation is solved for ln(n_e * mean energy)
        ln_energy_density = fem.Expression("std::log(a) + b", a=self.energy, b=self.dens_before[e], degree=1)
        self.w_now, self.w_before = fem.interpolate(ln_energy_density, V), fem.interpolate(ln_energy_density, V)
        self.w_before2 = fem.interpolate(fem.Constant(0.0), V)
        for k, name in enumerate(deck["file_names"]):
            self.scratch.assign(self.dens_before[k])
            self.scratch.rename(name, str(k))
            writers["density"][k].write_checkpoint(self.scratch, name, t * 1e6, fem.XDMFFile.Encoding.HDF5, False)

    def refresh_tables(self, deck, status):
        """Nodal transport and rate coefficients from the tables, at the mean energy / reduced field of
        the last accepted step; on updates also the table slopes the semi-implicit terms multiply."""
        energy = self.energy if status == "initial" else self.energy_before
        first = (self.mu,) if status == "initial" else ()
        fedm.Transport_coefficient_interpolation(status, deck["mu_dep"], GAS_DENSITY, GAS_TEMPERATURE, self.mu,
                                                 deck["mu_x"], deck["mu_y"], energy, self.field, *first)
        fedm.Transport_coefficient_interpolation(status, deck["D_dep"], GAS_DENSITY, GAS_TEMPERATURE, self.D,
                                                 deck["D_x"], deck["D_y"], energy, self.field, self.mu)
        fedm.Rate_coefficient_interpolation(status, deck["k_dep"], self.k, deck["k_x"], deck["k_y"], energy,
                                            self.field, Te=0, Tgas=0)
        if status == "initial":
            return
        e, at = deck["n_species"] - 1, self.energy_before.vector()[:]
        for j, dep in enumerate(deck["k_dep"]):
            if dep == "Umean":
                self.dk[j].vector()[:] = np.interp(at, deck["k_x"][j], deck["dk"][j])
        self.dmu[e].vector()[:] = np.interp(at, deck["mu_x"][e], deck["dmu_e"])
        self.dD[e].vector()[:] = np.interp(at, deck["D_x"][e], deck["dD_e"])


def electrode_conditions(space, powered_value):
    def powered(x, on_boundary):
        return on_boundary and fem.near(x[1], 0, fem.DOLFIN_EPS)

    def grounded(x, on_boundary):
        return on_boundary and fem.near(x[1], GAP, fem.DOLFIN_EPS)
    return [fem.DirichletBC(space, powered_value, powered), fem.DirichletBC(space, fem.Constant(0.0), grounded)]


def starting_potential(dis, deck, r, voltage, writers, t):
    """Poisson's equation for the uniform start (zero net charge) with the electrode values at t = 0."""
    charge = sum(elementary_charge * z * fem.exp(n) for z, n in zip(deck["charge_numbers"], dis.dens_before))
    form = fedm.weak_form_Poisson_equation(fem.dx, fem.TrialFunction(dis.scalar), fem.TestFunction(dis.scalar),
                                           charge / (fem.Constant(1.0) * epsilon_0), r)
    conditions = electrode_conditions(dis.scalar, voltage)
    matrix, load = fem.assemble(fem.lhs(form), tensor=None), fem.assemble(fem.rhs(form), tensor=None)
    for condition in conditions:
        condition.apply(matrix)
        condition.apply(load)
    fem.solve(matrix, dis.phi.vector(), load, "mumps")
    dis.phi_before2.assign(dis.phi_before)
    dis.phi_before.assign(dis.phi)
    dis.scratch.assign(dis.phi)
    dis.scratch.rename("Phi", str(0))
    writers["potential"] << (dis.scratch, t)


def coupled_form(dis, deck, mesh, r, dt, dt_before, wall_tags):
    """Energy balance (row 0), particle balances (rows 1..3), Poisson (row 4), in logarithmic variables,
    with the coefficients linearised around the last step's mean energy (semi-implicit)."""
    ns, neq = deck["n_species"], deck["n_equations"]
    e, i_phi = ns - 1, neq - 1
    u, v, Z = dis.trial, dis.tests, deck["charge_numbers"]
    ds = fem.Measure("ds", domain=mesh, subdomain_data=wall_tags)
    outward = fem.FacetNormal(mesh)
    E = -fem.grad(u[i_phi])
    # mean energy of the new step from the unknowns, linearised: eps_old + (w - n_e eps_old) / n_e,old
    energy_new = dis.energy_before + (fem.exp(u[0]) - fem.exp(u[e]) * dis.energy_before) / fem.exp(dis.dens_before[e])
    k = fedm.semi_implicit_coefficients(deck["k_dep"], energy_new, dis.energy_before, dis.k, dis.dk)
    mu = fedm.semi_implicit_coefficients(deck["mu_dep"], energy_new, dis.energy_before, dis.mu, dis.dmu)
    D = fedm.semi_implicit_coefficients(deck["D_dep"], energy_new, dis.energy_before, dis.D, dis.dD)
    gradient_of_nD = [role == "electrons" for role in CHARGE_ROLE]            # electrons: flux = -grad(D n)

    def drift_diffusion(j, unknown, scale=1.0):
        d_j, mu_j = (D[j], mu[j]) if scale == 1.0 else (scale * D[j] / 3.0, scale * mu[j] / 3.0)
        return fedm.Flux(Z[j], unknown, d_j, mu_j, E, grad_diffusion=gradient_of_nD[j], logarithm_representation=True)

    fluxes = [0] + [drift_diffusion(j, u[j]) for j in range(1, ns)]
    ions_to_wall = sum(fedm.Max(fem.dot(fluxes[j], outward), 0) for j in range(1, ns) if CHARGE_ROLE[j] == "Ion")
    energy_flux = drift_diffusion(e, u[0], scale=5.0)
    thermal_speed = [0] + [np.sqrt(8.0 * kB * GAS_TEMPERATURE / (fem.pi * deck["masses"][j])) for j in range(1, e)]
    thermal_speed.append(fem.sqrt(16.0 * elementary_charge * dis.energy / (3.0 * fem.pi * deck["masses"][e])))

    sources = fedm.Source_term("coupled", "LMEA", deck["power"], deck["loss"], deck["gain"], k, GAS_DENSITY, u)
    heating = fedm.Energy_Source_term("coupled", deck["power"], deck["loss"], deck["gain"], k, deck["energy_loss"],
                                      u[0] / u[e], GAS_DENSITY, u)
    heating += -fem.dot(drift_diffusion(e, u[e]), E)                          # Joule heating

    form = 0
    for j in range(1, ns):
        form += fedm.weak_form_balance_equation_log_representation(
            KINDS[j], dt, dt_before, fem.dx, u[j], dis.before[j], dis.before2[j], v[j], sources[j], fluxes[j], r, D[j])
    for tag, (reflect, emit) in enumerate(zip(REFLECTION, SECONDARY_EMISSION), start=1):
        for j in range(1, ns):
            form += fedm.Boundary_flux("flux source", KINDS[j], WALL_ROLE[j], Z[j], mu[j], E, outward, u[j], emit,
                                       v[j], ds(tag), r, thermal_speed[j], reflect[j], ions_to_wall)
    energy_form = fedm.weak_form_balance_equation_log_representation(
        KINDS[e], dt, dt_before, fem.dx, u[0], dis.before[0], dis.before2[0], v[0], heating, energy_flux, r)
    emitted_energy = fem.Expression("u_p", u_p=SECONDARY_ENERGY, degree=1)
    for tag, (reflect, emit) in enumerate(zip(REFLECTION, SECONDARY_EMISSION), start=1):
        energy_form += fedm.Boundary_flux("flux source", KINDS[e], WALL_ROLE[e], Z[e], 5.0 * mu[e] / 3.0, E, outward,
                                          u[0], emit * emitted_energy, v[0], ds(tag), r, 1.3333 * thermal_speed[e],
                                          reflect[e], ions_to_wall)
    form += energy_form
    space_charge = sum(elementary_charge * z * fem.exp(u[j]) for j, z in enumerate(Z))
    form += fedm.weak_form_Poisson_equation(fem.dx, u[i_phi], v[i_phi], space_charge / (fem.Constant(1.0) * epsilon_0), r)
    return form


def balance_columns(names):
    """The columns of a `--balance` row for the species `names` (the gas first; its place is the energy's)."""
    what = ["energy"] + list(names[1:])
    return (["t"] + [f"content_{n}" for n in what] + ["current_powered", "current_grounded", "power_joule",
            "collision_loss"] + [f"imbalance_{n}" for n in what] + ["current_ramo"])


def balance_row(t, b):
    """One `--balance` row from a `fedm_amd.device.Balance`: SI units, currents in A, power in W, the loss in eV/s."""
    return [t, *b.content, b.wall_current[0], b.wall_current[1], b.power_joule, b.collision_loss, *b.imbalance, b.current]


CURRENTS_COLUMNS = ("t", "conduction_powered", "displacement_powered", "total_powered", "conduction_grounded",
                    "displacement_grounded", "total_grounded")


def currents_row(t, c):
    """One `--currents` row from a `fedm_amd.device.Currents`: t, then conduction, displacement and total [A] per electrode."""
    return [t] + [x for g in range(len(c.conduction)) for x in (c.conduction[g], c.displacement[g], c.total[g])]


CIRCUIT_COLUMNS = ("t", "V_s", "U", "lead_current", "conduction", "conductance")


def main(nx=100, ny=100, T_final=1e-11, input_dir=None, output_dir="gd_output", quiet=True, ttol=2e-3,
         stop_before_device=None, balance=None, balance_every=1, fields=None, fields_every=1, axis_profile=None,
         currents=None, currents_every=1, ballast=None, stray_capacitance=0.0, circuit_log=None):
    fem.parameters["form_compiler"]["quadrature_degree"] = 4
    deck = read_deck(input_dir)
    file_io.files.output_folder_path = Path(output_dir)
    ns, neq = deck["n_species"], deck["n_equations"]
    writers = {"density": file_io.output_files("xdmf", "number density", deck["file_names"]),
               "potential": file_io.output_files("pvd", "potential", ["Phi"])[0]}
    t = 0.0
    dt = fem.Expression("time_step", time_step=1e-13, degree=0)
    dt_before = fem.Expression("time_step", time_step=1e30, degree=0)
    dt_limits = dict(dt_min=1e-15, dt_max=1e-8)
    r = fem.Expression("x[0]", degree=1)
    file_io.log("conditions", file_io.files.model_log, dt.time_step, VOLTAGE, PRESSURE, GAP, GAS_DENSITY, GAS_TEMPERATURE)
    file_io.log("properties", file_io.files.model_log, "Ar", DECK, deck["file_names"], deck["masses"],
                [z * elementary_charge for z in deck["charge_numbers"]])

    mesh = fem.RectangleMesh((0, 0), (RADIUS, GAP), nx, ny, "crossed")
    wall_tags = fedm.Marking_boundaries(mesh, SIDES)
    file_io.log("matrices", file_io.files.model_log, deck["gain"], deck["loss"], deck["power"])
    file_io.log("initial time", file_io.files.model_log, t)
    dis = Discharge(mesh, deck)
    dis.start(deck, writers, t)
    voltage = fem.Expression("U0*(1-exp(-t/1e-9))", U0=VOLTAGE, t=t, pi=fem.pi, degree=0)    # switched on with a 1 ns rise
    starting_potential(dis, deck, r, voltage, writers, t)
    dis.field.assign(reduced_field(dis.phi))
    dis.field_before.assign(dis.field)
    dis.refresh_tables(deck, "initial")

    form = coupled_form(dis, deck, mesh, r, dt, dt_before, wall_tags)
    parts_now = [dis.w_now] + dis.dens_now[1:] + [dis.phi]
    parts_before = [dis.w_before] + dis.dens_before[1:] + [dis.phi_before]
    parts_before2 = [dis.w_before2] + dis.dens_before2[1:] + [dis.phi_before2]
    for mixed, parts in ((dis.now, parts_now), (dis.before, parts_before), (dis.before2, parts_before2)):
        dis.join.assign(mixed, parts)
    residual = fem.action(form, dis.now)
    jacobian = fem.derivative(residual, dis.now, dis.trial)
    problem = (stop_before_device or fedm.Problem)(jacobian, residual, electrode_conditions(dis.mixed.sub(neq - 1), voltage))

    # the device's linear solver (PETSc's defaults in a FEDM script): multigrid on the potential block,
    # Chebyshev(8) sweeps on the species block (tools/gd_cycle.py)
    from fedm_amd.device import chebyshev_weights
    problem.device.setup_multigrid(nu=1)
    problem.device.set_fieldsplit(chebyshev_weights(8, 0.3, 2.2))
    newton = fedm.PETScSNESSolver()
    newton.parameters.update(relative_tolerance=1e-4, linear_solver="mumps")     # iteration limit: the solver's default

    out_files = [writers["potential"]] + writers["density"][1:]
    out_names = ["Phi"] + deck["file_names"][1:]
    out_now, out_before = [dis.phi] + dis.dens_now[1:], [dis.phi_before] + dis.dens_before[1:]
    window, stride = OUTPUT_WINDOWS[0], OUTPUT_STRIDES[0]
    balance_of, rows = None, None
    if balance is not None:
        balance_of = fedm.Discharge_balance(problem, boundary_tags=(1, 2), weighting_potential=problem.device.coords[:, 1] / GAP)
        rows = open(balance, "w")
        rows.write("# " + " ".join(balance_columns(deck["file_names"])) + "\n")
    currents_of = current_rows = None
    if currents is not None:
        currents_of = fedm.Electrode_currents(problem, boundary_tags=(1, 2))
        current_rows = open(currents, "w")
        current_rows.write("# " + " ".join(CURRENTS_COLUMNS) + "\n")
    circuit = circuit_rows = None
    timed = [voltage]
    if ballast is not None:
        # the powered electrode (tag 1) behind the ballast and its stray capacitance, the grounded one (tag 2) ideal
        electrodes = currents_of or fedm.Electrode_currents(problem, boundary_tags=(1, 2))
        circuit = fedm.External_circuit(problem, electrodes, [lambda s: VOLTAGE * (1.0 - np.exp(-s / 1e-9)), lambda s: 0.0],
                                        [float(ballast), 0.0], [float(stray_capacitance), 0.0]).bind(problem)
        timed = [voltage, circuit]
        if circuit_log is not None:
            circuit_rows = open(circuit_log, "w")
            circuit_rows.write("# " + " ".join(CIRCUIT_COLUMNS) + "\n")
    field_out = field_files = profile = profile_rows = None
    if fields:
        fields = [name.strip() for name in (fields.split(",") if isinstance(fields, str) else fields) if name.strip()]
        field_out = fedm.Field_output(problem, fields, species_names=deck["file_names"])
        field_files = file_io.output_files("pvd", "fields", [name.replace(":", "_") for name in fields])
        for writer in field_files:
            writer.mesh = mesh
    if axis_profile is not None:
        # its own set-up on the same problem: the requests go with a call, the points belong to the context
        z_axis = np.linspace(0.0, GAP, AXIS_POINTS)
        profile = fedm.Field_output(problem, AXIS_FIELDS, probes=np.column_stack([0.0 * z_axis, z_axis]),
                                    species_names=deck["file_names"])
        profile_rows = open(axis_profile, "w")
        profile_rows.write("# t, then %s at %d points each on r = 0; first row: nan and the points' z per field\n"
                           % (", ".join(AXIS_FIELDS), AXIS_POINTS))
        profile_rows.write(" ".join(f"{x:.17g}" for x in [float("nan"), *np.tile(z_axis, len(AXIS_FIELDS))]) + "\n")
    field_window, field_stride, outputs = OUTPUT_WINDOWS[0], OUTPUT_STRIDES[0], 0
    step_errors, recent_errors, steps = [0.0] * (ns + 1), [1] * 3, 0
    while t < T_final:
        t_before = t
        dis.before2.assign(dis.before)
        dis.before.assign(dis.now)
        dis.split.assign(parts_before, dis.before)
        dis.field_before.assign(dis.field)
        dis.energy_before2.assign(dis.energy_before)
        dis.energy_before.assign(dis.energy)
        dis.field.assign(reduced_field(dis.phi))
        dis.refresh_tables(deck, "update")
        with contextlib.redirect_stdout(io.StringIO() if quiet else sys.stdout):
            t = fedm.adaptive_solver(newton, problem, t, dt, dt_before, dis.now, dis.before, parts_now, parts_before,
                                     dis.split, step_errors, file_io.files.error_file, recent_errors, ttol,
                                     dt_limits["dt_min"], time_dependent_arguments=timed, approximation="LMEA")
        file_io.log("time", file_io.files.model_log, t)
        if circuit is not None:     # the accepted step: the history moves on, conduction and conductance of the new state
            circuit.accept()
            if circuit_rows is not None:
                circuit_rows.write(" ".join(repr(v) for v in circuit.log_row(t, 0)) + "\n")
                circuit_rows.flush()
        if balance_of is not None and steps % max(1, int(balance_every)) == 0:
            # (here, before anything of the next step reaches the device: the balance of the residual just solved)
            rows.write(" ".join(repr(float(v)) for v in balance_row(t, balance_of())) + "\n")
            rows.flush()
        if currents_of is not None and steps % max(1, int(currents_every)) == 0:     # (here too: the residual just solved)
            current_rows.write(" ".join(repr(float(v)) for v in currents_row(t, currents_of())) + "\n")
            current_rows.flush()
        if profile is not None:     # (here too: the state and the table of the residual just solved)
            p = profile()["probes"]
            profile_rows.write(" ".join(f"{x:.17g}" for x in [t, *p.ravel()]) + "\n")
            profile_rows.flush()
        if field_out is not None:
            from fedm_amd.mesh_io import output_times
            due, (field_window, field_stride) = output_times(t, field_window, field_stride, OUTPUT_WINDOWS, OUTPUT_STRIDES)
            if due:                 # one set per accepted step that reaches an output time, at the step's own time
                outputs += 1
                if outputs % max(1, int(fields_every)) == 0:
                    values = field_out()
                    for name, writer in zip(fields, field_files):
                        writer.write(values[name], name, t)
        dis.energy.vector()[:] =np.exp(dis.w_now.vector()[:] - dis.dens_now[ns - 1].vector()[:])
        window, stride = file_io.file_output(t, t_before, window, stride, OUTPUT_WINDOWS, OUTPUT_STRIDES,
                                             ["pvd"] + ["xdmf"] * (ns - 1), out_files, out_names, out_now, out_before,
                                             unit="us")
        dt_before.time_step = dt.time_step
        dt.time_step = fedm.adaptive_timestep(dt.time_step, recent_errors, ttol, **dt_limits)
        recent_errors[1:] = recent_errors[:2]
        steps += 1
    if rows is not None:
        rows.close()
    if profile_rows is not None:
        profile_rows.close()
    if current_rows is not None:
        current_rows.close()
    if circuit_rows is not None:
        circuit_rows.close()
    return dict(t=t, steps=steps, output=str(file_io.files.output_folder_path), species=deck["file_names"],
                error_file=str(file_io.files.error_file), problem=problem)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out", nargs="?", default="gd_output")
    ap.add_argument("--balance", metavar="FILE", help="write the particle and energy balance per accepted step")
    ap.add_argument("--balance-every", type=int, default=1, metavar="N", help="... every N-th accepted step")
    ap.add_argument("--currents", metavar="FILE",
                    help="write t and the conduction, displacement and total current of both electrodes per accepted step")
    ap.add_argument("--currents-every", type=int, default=1, metavar="N", help="... every N-th accepted step")
    ap.add_argument("--ballast", type=float, metavar="OHMS",
                    help="run the powered electrode behind a series resistor (fedm.External_circuit); off by default")
    ap.add_argument("--stray-capacitance", type=float, default=0.0, metavar="F", help="... with this capacitance to ground in parallel")
    ap.add_argument("--circuit-log", metavar="FILE",
                    help="... and write %s of the powered electrode per accepted step" % ", ".join(CIRCUIT_COLUMNS))
    ap.add_argument("--fields", metavar="LIST",
                    help="comma-separated derived fields written at the output times: mean_energy, reduced_field, E_norm, "
                         "E_r, E_z, charge, density:s, state:e, table:f, rate:j, source:s, collision_loss, joule, "
                         "flux_r:s, flux_z:s, current_r, current_z (s: a species' index or name; 0 is the energy)")
    ap.add_argument("--fields-every", type=int, default=1, metavar="N", help="... at every N-th output time")
    ap.add_argument("--axis-profile", metavar="FILE", help="write the profiles of %s on r = 0 per accepted step" % ", ".join(AXIS_FIELDS))
    a = ap.parse_args()
    result = main(output_dir=a.out, quiet=False, balance=a.balance, balance_every=a.balance_every, fields=a.fields,
                  fields_every=a.fields_every, axis_profile=a.axis_profile, currents=a.currents,
                  currents_every=a.currents_every, ballast=a.ballast, stray_capacitance=a.stray_capacitance,
                  circuit_log=a.circuit_log)
    print({k: v for k, v in result.items() if k != "problem"})
