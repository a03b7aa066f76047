"""Small synthetic LMEA models, meshes and states that span the family of ``fedm_gd_desc`` (helper module of
test_lmea_family_reference.py and test_gpu_lmea_family.py).  No deck files: a model is a ``GdModel``, its nodal field table
is made here and goes in through ``DeviceProblem.set_gd_fields``.

Scaling.  Every addend of the residual has to be visible at the bounds the device is held to, so the states are balanced
on purpose around one rate X = 5e7 / s (the BDF2 term of a 2 % change in 1.1 ns):
  * ``charge_over_eps`` is the physical 1.8e-8 V m: densities near e^34 (5e14 / m^3) put the charge parts of the Poisson
    row beside its gradient part for a field of 1e4 V/m on millimetre cells.  (At that field Joule heating, mu E^2 n_e,
    balances the energy row's me n_e X with a mean energy me = E h of a few eV, and the sentinel losses -- Ei - u_0 / u_e
    and u_0 / u_e itself, numbers of order 1 .. 15 whatever the densities are -- stand beside the deck-like losses.)
  * mobilities mu = X h / E, diffusion coefficients D = 1.5 X h^2 (h: the mesh's cell size), heavy thermal velocities
    X h0 with h0 = 1 mm; ``electron_mass`` is chosen so that sqrt(vth_e_coef me) = 2 X h0; each reaction's k so that its
    rate is X times a typical density; N0 = 1e20.
  * u_e is near 34 and u_0 = ln(me) + u_e, so u_0 / u_e is near 1.03; me > 0 (3 eV +- 10 %).
Every row of the field table is non-zero and non-constant, the mu_d, D_d and kd rows of every species and reaction
included (a tenth of the row they belong to per eV, alternating in sign).

The sixth member of the family, `deck-degree6`, is the argon deck itself at quadrature degree 6 (no table of exponentials
on the production model): tests/test_balance_reference.perturbed_case("deck", 6) with the oracle behind it.

Meshes on r in [2 mm, 2 mm + L], z in [0, L] (off the axis, so that all four walls carry weight): tags 1 .. 4 = bottom,
top, inner, outer; the potential is constrained on the bottom and the top.
"""
import sys
import types
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

X_RATE, FIELD, H0, N0, R0, GAP = 5e7, 1e4, 1e-3, 1e20, 2e-3, 1e-2
S1, S2 = 7.77e77, 9.99e99
RX, DR, DD = "reaction", "diffusion-reaction", "drift-diffusion-reaction"

# id -> species after the gas (name, eq_type, grad_diffusion, is_ion, sign) and reactions (power, net, energy loss), both
# over all species, the gas first
MODELS = {
    "e-only": dict(
        species=[("e", DD, True, False, -1.0)],
        reactions=[([1, 1], [0, 1], 11.55)]),
    "ion-e": dict(
        species=[("A+", DD, True, True, 1.0), ("e", DD, False, False, -1.0)],
        reactions=[([1, 0, 1], [0, 1, 1], 15.76),
                   ([2, 0, 2], [-1, 1, 1], -3.0),          # electron power 2, gas power 2
                   ([0, 1, 1], [1, -1, -1], 2.5)]),
    "deck-shape-permuted": dict(
        species=[("B-", DD, False, True, -1.0), ("M", RX, False, False, 0.0), ("e", DD, True, False, -1.0)],
        reactions=[([1, 0, 0, 1], [0, 0, 1, 0], 11.55),
                   ([1, 0, 0, 1], [0, 0, 0, 1], S1),
                   ([0, 0, 4, 0], [0, 0, -2, 1], -7.34),   # a power of 4: the rolled loop
                   ([1, 0, 0, 1], [0, 1, 0, -1], 4.21),
                   ([1, 0, 0, 1], [0, 0, 0, 0], S2)],
        energy_Ei=15.76, mean_energy_form="unknown_ratio"),
    "two-ions-small": dict(
        species=[("M", DR, False, False, 0.0), ("A+", DD, True, True, 1.0), ("B-", DD, False, True, -1.0),
                 ("e", DD, True, False, -1.0)],
        reactions=[([1, 0, 0, 0, 1], [0, 0, 1, 0, 1], 15.76),
                   ([1, 0, 0, 0, 1], [0, 1, 0, 1, -1], 11.55),
                   ([0, 1, 1, 1, 0], [1, -1, -1, -1, 0], 1.0)]),
    # (the reactions are written in the order gas, M, A+, B-, e of two-ions-small; `_FULL_ORDER` then puts the positive
    # ion first, so that the diffusion-reaction species sits at index 2 -- the deck and two-ions-small have it at 1)
    "two-ions-full": dict(
        species=[("M", DR, False, False, 0.0), ("A+", DD, True, True, 1.0), ("B-", DD, False, True, -1.0),
                 ("e", DD, True, False, -1.0)],
        reactions=[([1, 0, 0, 0, 1], [0, 0, 1, 0, 1], 15.76),
                   ([1, 0, 0, 0, 1], [-1, 1, 0, 0, 0], 11.55),
                   ([0, 1, 0, 0, 1], [0, -1, 1, 0, 1], 4.21),
                   ([0, 2, 0, 0, 0], [1, -2, 1, 0, 1], -7.34),
                   ([1, 0, 0, 0, 1], [0, 0, 0, 1, -1], S1),
                   ([1, 0, 0, 0, 1], [0, 0, 0, 0, 0], S2),
                   ([0, 0, 1, 1, 0], [0, 1, -1, -1, 0], 1.1),
                   ([0, 0, 1, 0, 2], [0, 1, -1, 0, -1], -3.0),    # electron power 2
                   ([2, 0, 0, 0, 1], [0, 0, 1, 0, 1], 12.0),      # gas power 2
                   ([0, 4, 0, 0, 0], [1, -3, 1, 0, 1], -1.0),     # a power of 4
                   ([0, 0, 0, 1, 1], [0, 0, 0, -1, 1], 1.5),
                   ([0, 1, 0, 1, 0], [1, -1, 0, -1, 1], 0.7),
                   ([1, 0, 1, 0, 0], [0, 1, -1, 0, 0], 0.9),
                   ([0, 0, 2, 0, 0], [1, 0, -1, 0, 0], 0.8),
                   ([0, 0, 0, 2, 1], [0, 1, 0, -2, 0], 2.2),
                   ([1, 1, 0, 0, 1], [0, -1, 0, 1, 0], 3.3)],
        energy_Ei=15.76, mean_energy_form="unknown_ratio"),
}
_FULL_ORDER = [0, 2, 1, 3, 4]
_full = MODELS["two-ions-full"]
_full["species"] = [_full["species"][i - 1] for i in _FULL_ORDER[1:]]
_full["reactions"] = [([p[i] for i in _FULL_ORDER], [n[i] for i in _FULL_ORDER], loss) for p, n, loss in _full["reactions"]]
# reflection coefficients of the four tags: distinct rows; tag 2 reflects one species completely (ref = 1: the first after the gas, the
# negative ion where there are two ions), tag 3 reflects nothing (ref = 0); the outer wall emits nothing (gamma = 0)
REF_ROWS = [[0.30, 0.10, 0.20, 0.25, 0.15], [0.05, 0.40, 0.35, 0.12, 0.22], [0.0] * 5, [0.50, 0.60, 0.45, 0.55, 0.65]]
GAMMA = [0.06, 0.10, 0.03, 0.0]
WE_SECONDARY = 5.0
MESHES = ("3x3", "10x10", "irregular")
IRREGULAR_FOR = ("deck-shape-permuted", "two-ions-full")      # the models that also run on the irregular mesh
PLANAR_TOO = ("e-only", "two-ions-small")
# which of tests/lmea_family_reference.PERTURBATIONS apply to which model (it has the feature the fault is in);
# test_lmea_family_reference.py holds this table to the perturbations' own `applies` and each entry to its bound
_ALWAYS = ["tag t's ref taken from tag t - 1", "the kd of one reaction dropped", "planar and axisymmetric weights swapped",
           "the 5/3 of the energy flux applied to D only"]
_ION = ["gamma not scaled by we_secondary in the energy row", "an ion's mu_d * dme dropped",
        "a heavy species' D_d * dme dropped"]
_TWO_IONS = _ION + ["an ion's grad_diffusion term dropped", "second ion left out of the emission sum"]
APPLIES = {
    "e-only": _ALWAYS,
    "ion-e": _ALWAYS + _ION + ["an ion's grad_diffusion term dropped", "electron power 2 differentiated as 1"],
    "deck-shape-permuted": _ALWAYS + _ION + ["a power of 4 taken as 3", "a reaction-type species given a flux",
                                             "sentinel kind-1 weight loses Ei"],
    "two-ions-small": _ALWAYS + _TWO_IONS,
    "two-ions-full": _ALWAYS + _TWO_IONS + ["a power of 4 taken as 3", "electron power 2 differentiated as 1",
                                            "sentinel kind-1 weight loses Ei"],
}


def model(name, planar=False, degree=4):
    from fedm_amd.device import GdModel
    from fedm_amd.physical_constants import elementary_charge
    spec = MODELS[name]
    sp = [("gas", RX, False, False, 0.0)] + spec["species"]
    ns = len(sp)
    ref = [row[:ns] for row in REF_ROWS]
    ref[1][1 if ns <= 4 else 3] = 1.0
    vth_e_coef = (2.0 * X_RATE * H0) ** 2 / 3.0
    return GdModel(n_species=ns, N0=N0, eq_type=[s[1] for s in sp], grad_diffusion=[s[2] for s in sp],
                   is_ion=[s[3] for s in sp], sign=[s[4] for s in sp],
                   vth=[0.0] + [X_RATE * H0 * (1.0 + 0.1 * i) for i in range(1, ns - 1)] + [0.0],
                   electron_mass=16.0 * elementary_charge / (3.0 * np.pi * vth_e_coef),
                   power=[r[0] for r in spec["reactions"]], net=[r[1] for r in spec["reactions"]],
                   energy_loss=[r[2] for r in spec["reactions"]], ref=ref, gamma=list(GAMMA), we_secondary=WE_SECONDARY,
                   quadrature_degree=degree, axisymmetric=not planar, energy_Ei=spec.get("energy_Ei", 0.0),
                   mean_energy_form=spec.get("mean_energy_form"))


_MESHES = {}


def mesh(name):
    """namespace(coords, cells, tags, bottom, top, L): the vertices of the two constrained sides by number"""
    from oracle import mesh as omesh
    if name in _MESHES:
        return _MESHES[name]
    if name == "3x3":         # 18 cells: one workgroup, 46 of its 64 lanes without a cell; corner cells with two tagged facets
        m, L = omesh.rectangle_right(R0, 0.0, R0 + GAP, GAP, 3, 3), GAP
    elif name == "10x10":     # 400 cells: seven workgroups, the last with 16 cells
        m, L = omesh.rectangle_crossed(R0, 0.0, R0 + GAP, GAP, 10, 10), GAP
    elif name == "irregular":  # a 24 x 30 grid with a wheel of 11 spokes in it: row widths and contribution counts vary
        import limit_meshes
        coords, cells = limit_meshes._ring(24, 30, (1, 2, 1, 2), 1, (12, 15))
        L = limit_meshes.BOX
        m = omesh.Mesh(coords + np.array([R0, 0.0]), cells)
    else:
        raise KeyError(name)
    r1 = float(m.coords[:, 0].max())
    tags = omesh.mark_boundaries(m, [["line", 0.0, 0.0, R0, r1], ["line", L, L, R0, r1], ["line", 0.0, L, R0, R0],
                                     ["line", 0.0, L, r1, r1]])
    z = m.coords[:, 1]
    out = types.SimpleNamespace(coords=m.coords, cells=m.cells, tags=tags, L=L, nv=m.nv, nc=m.nc,
                                bottom=np.nonzero(np.abs(z) <= 3e-16)[0], top=np.nonzero(np.abs(z - L) <= 3e-16)[0])
    for a in (out.coords, out.cells, out.tags):
        a.setflags(write=False)
    _MESHES[name] = out
    return out


def rules(degree):
    from fedm_amd import quadrature
    return quadrature.triangle(degree), quadrature.interval(degree)


_CASES = {}


def case(name, mesh_name="10x10", planar=False, degree=4):
    """The model, its mesh, field table and states: namespace(model, md, mesh, fields, U, Uo, Uo1, dt, dt_old,
    dirichlet_dofs, dirichlet_vals, rules).  Made once per argument list and read-only from then on."""
    key = (name, mesh_name, planar, degree)
    if key in _CASES:
        return _CASES[key]
    gm = model(name, planar, degree)
    g = mesh(mesh_name)
    ns, nr, nv = gm.n_species, gm.n_reactions, g.nv
    ie, neq = ns - 1, ns + 1
    h = float(np.sqrt(2.0 * g.L * g.L / g.nc))
    rng = np.random.default_rng(sum(map(ord, name)) + 131 * g.nc)
    xh, yh = (g.coords[:, 0] - R0) / g.L, g.coords[:, 1] / g.L

    def vary(k):
        return 1.0 + 0.2 * np.sin((2.0 + 0.7 * k) * xh + 0.9 * k) * np.cos((1.5 + 0.4 * k) * yh + 0.3 * k) \
            + 0.05 * rng.uniform(-1.0, 1.0, nv)

    me_old = 3.0 * vary(1)
    me = me_old + rng.normal(0, 0.05, nv)
    ubar = [np.log(N0)] + [34.0 + 0.25 * ((3 * i) % 4 - 1.5) for i in range(1, ns)]
    U = np.zeros((nv, neq))
    for i in range(1, ns):
        U[:, i] = ubar[i] + rng.normal(0, 0.2, nv)
    U[:, 0] = np.log(me) + U[:, ie] + rng.normal(0, 0.05, nv)
    U[:, ns] = -FIELD * g.L * (1.0 - yh) + rng.normal(0, 0.3 * FIELD * h, nv)
    Uo = U + rng.normal(0, 0.02, U.shape)
    Uo1 = U + rng.normal(0, 0.02, U.shape)
    rows, row = [], 0
    mu0, D0 = X_RATE * h / FIELD, 1.5 * X_RATE * h * h
    base = [mu0 * (1.0 + 0.15 * i) for i in range(ns)] + [D0 * (1.0 + 0.1 * i) for i in range(ns)]
    for b in base:
        rows.append(b * vary(row))
        row += 1
    for b in base:                          # mu_d, D_d: a tenth per eV, alternating in sign
        rows.append((0.1 if row % 2 else -0.1) * b * vary(row))
        row += 1
    n_typ = float(np.exp(34.0))
    ks = []
    for j in range(nr):
        prod = 1.0
        for i in range(ns):
            prod *= float(np.exp(ubar[i])) ** gm.power[j][i]
        ks.append(X_RATE * n_typ / prod * (1.0 + 0.1 * (j % 5)))
    for k in ks:
        rows.append(k * vary(row))
        row += 1
    for j, k in enumerate(ks):
        rows.append((0.1 if j % 2 else -0.1) * k * vary(row))
        row += 1
    fields = np.stack(rows + [me_old, me, Uo[:, ie].copy()])
    assert fields.shape[0] == gm.n_fields
    ddofs = np.concatenate([g.bottom, g.top]) * neq + ns
    dvals = np.concatenate([np.full(g.bottom.size, -0.97 * FIELD * g.L), np.full(g.top.size, 1.5)])
    out = types.SimpleNamespace(name=name, model=gm, md=gm.to_c(), mesh=g, fields=fields, U=U, Uo=Uo, Uo1=Uo1, dt=1.1e-9,
                                dt_old=0.7e-9, dirichlet_dofs=ddofs, dirichlet_vals=dvals, rules=rules(degree), h=h)
    for a in (fields, U, Uo, Uo1, ddofs, dvals):
        a.setflags(write=False)
    _CASES[key] = out
    return out


def restate(c, **kw):
    """tests/lmea_family_reference.residual_jacobian at the case"""
    import lmea_family_reference as fam
    return fam.residual_jacobian(c.md, c.mesh.coords, c.mesh.cells, c.mesh.tags, c.fields, c.U, c.Uo, c.Uo1, c.dt, c.dt_old,
                                 c.dirichlet_dofs, c.dirichlet_vals, c.rules, **kw)
