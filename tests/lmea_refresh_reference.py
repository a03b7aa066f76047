"""One per-step refresh of the LMEA coefficient fields, restated in float64 numpy/scipy (test infra).

Written from the formulas of the script and the library it drives, not from the device code:

* examples/glow_discharge/fedm-gd.py:424-443 -- ``u_oldV`` is taken from the previous state, ``mean_energy_old`` takes
  ``mean_energy``, ``redE = project(1e21*sqrt(dot(-grad(Phi), -grad(Phi)))/N0)``, then the transport and rate
  coefficients are interpolated at the OLD mean energy or at redE, and the derivative tables at the old mean energy;
* fedm/functions.py:621-637 -- ``np.interp(arg, kx, ky) / N0`` for 'Umean' and 'E/N', ``kB*Tgas*mu/e`` for 'ESR' (a
  row scaled from another row, so it comes after the look-ups), nothing for 'const';
* fedm/functions.py:724-748 -- ``np.interp(arg, kx, ky)`` for the rate coefficients;
* fedm-gd.py:452 -- ``mean_energy = exp(u_0 - u_e)`` after the solve.

The field rows are those of ``DeviceProblem.set_gd_fields`` (FEDM_GD_N_FIELDS): mu, D, mu_diff, D_diff per species,
k, k_diff per reaction, mean_energy_old, mean_energy, u_e_old; the programs are the dicts of
``DeviceProblem.gd_prep_setup``.  ``project`` of a cell-wise constant onto P1 is the consistent mass solve, done here
by sparse LU; :func:`jacobi_cg` is the textbook Jacobi-preconditioned CG, kept only to measure how far that
ALGORITHM sits from LU at the tolerance the device uses (1e-14, at most 500 iterations).
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = Path(__file__).resolve().parent.parent
DECK = ROOT / "decks" / "glow_discharge" / "file_input"
kB, elementary_charge = 1.38064852e-23, 1.6021766208e-19


# ---- the projection -------------------------------------------------------------------------------------------------
def _geometry(coords, cells):
    x = np.asarray(coords, dtype=np.float64)[np.asarray(cells)]
    d1, d2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    return x, d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]


def mass_matrix(coords, cells):
    """Consistent P1 mass matrix of ``u*v*dx`` (Cartesian measure, as ``project`` uses it): |det| / 24 * (1 + delta)."""
    _, det = _geometry(coords, cells)
    nv = np.asarray(coords).shape[0]
    vals = np.abs(det)[:, None, None] * ((np.ones((3, 3)) + np.eye(3)) / 24.0)[None]
    c = np.asarray(cells, dtype=np.int64)
    rows = np.broadcast_to(c[:, :, None], vals.shape).ravel()
    cols = np.broadcast_to(c[:, None, :], vals.shape).ravel()
    return sp.coo_matrix((vals.ravel(), (rows, cols)), shape=(nv, nv)).tocsr()


def reduced_field_rhs(coords, cells, N0, Phi):
    """int f v dx for the cell-wise constant f = 1e21 |grad Phi| / N0: f |det| / 6 to each vertex of a cell."""
    x, det = _geometry(coords, cells)
    P = np.asarray(Phi, dtype=np.float64)[np.asarray(cells)]
    # gradient of the P1 interpolant: sum_a Phi_a grad(lambda_a), grad(lambda_a) = rot(x_b - x_c) / det
    gx = (P[:, 0] * (x[:, 1, 1] - x[:, 2, 1]) + P[:, 1] * (x[:, 2, 1] - x[:, 0, 1])
          + P[:, 2] * (x[:, 0, 1] - x[:, 1, 1])) / det
    gy = (P[:, 0] * (x[:, 2, 0] - x[:, 1, 0]) + P[:, 1] * (x[:, 0, 0] - x[:, 2, 0])
          + P[:, 2] * (x[:, 1, 0] - x[:, 0, 0])) / det
    f = 1e21 * np.sqrt(gx * gx + gy * gy) / N0
    return np.bincount(np.asarray(cells).ravel(), weights=np.repeat(f * np.abs(det) / 6.0, 3),
                       minlength=np.asarray(coords).shape[0])


def reduced_field(coords, cells, N0, Phi, mass=None):
    M = mass_matrix(coords, cells) if mass is None else mass
    return spla.splu(M.tocsc()).solve(reduced_field_rhs(coords, cells, N0, Phi))


def jacobi_cg(M, b, rtol=1e-14, max_it=500):
    """Jacobi-preconditioned CG from x = 0, stopped at |r| <= rtol |b|: ``(x, iterations)``."""
    M = sp.csr_matrix(M)
    dinv = 1.0 / M.diagonal()
    x = np.zeros_like(b)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    rz, rr0 = r @ z, r @ r
    if rr0 == 0.0:
        return x, 0
    for it in range(1, max_it + 1):
        q = M @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if r @ r <= rtol * rtol * rr0:
            return x, it
        z = dinv * r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it


# ---- the refresh ----------------------------------------------------------------------------------------------------
def _row_of(programs, kind):
    (row,) = [r for r, p in enumerate(programs) if p["kind"] == kind]
    return row


def refresh(coords, cells, N0, tables, programs, fields, U, U_old):
    """``(fields_new, redE)`` of one refresh before a solve: U is the state the potential is taken from
    (its last column), U_old the previous one (its column n_eq - 2 is ln n_e of the previous step)."""
    U, U_old = np.asarray(U, dtype=np.float64), np.asarray(U_old, dtype=np.float64)
    n_eq = U.shape[1]
    redE = reduced_field(coords, cells, N0, U[:, n_eq - 1])
    new = np.array(fields, dtype=np.float64, copy=True)
    new[_row_of(programs, "me_old")] = new[_row_of(programs, "me")]      # first: the tables see the OLD mean energy
    args = {"energy": new[_row_of(programs, "me_old")], "redfield": redE}
    for r, p in enumerate(programs):
        if p["kind"] == "table":
            x, y = tables[p["table"]]
            new[r] = np.interp(args[p.get("arg", "energy")], x, y) * p.get("scale", 1.0)
        elif p["kind"] == "ue_old":
            new[r] = U_old[:, n_eq - 2]
    for r, p in enumerate(programs):                                     # 'ESR': from a row that was just refreshed
        if p["kind"] == "scaled_row":
            new[r] = p["scale"] * new[p["src_row"]]
    return new, redE


def mean_energy(U):
    U = np.asarray(U, dtype=np.float64)
    return np.exp(U[:, 0] - U[:, U.shape[1] - 2])


# ---- the deck's tables and programs, from the deck readers (no GPU) -----------------------------------------------
def read_deck(file_input=DECK, model="4_particles", Tgas=300.0, p0=1.0):
    """What ``fedm_amd.cases.glow_discharge.Case`` reads from the deck before it touches the device
    (fedm-gd.py:45-96), under the same attribute names."""
    from fedm_amd import file_io, functions as ff
    slot = "_dir_file_input"                          # (process-wide, as in the reference: put back below)
    before = file_io.files.__dict__.get(slot)
    file_io.files.file_input = Path(file_input)
    try:
        return _read_deck(file_io, ff, model, Tgas, p0)
    finally:
        if before is None:
            file_io.files.__dict__.pop(slot, None)
        else:
            file_io.files.__dict__[slot] = before


def _read_deck(file_io, ff, model, Tgas, p0):
    path = file_io.files.file_input / model
    d = SimpleNamespace(Tgas=Tgas, N0=p0 * 3.21877e22)
    ns, species, prop, names = file_io.read_speclist(path)
    M, sign = file_io.read_particle_properties(prop, model)
    kfiles = file_io.rate_coefficient_file_names(path)
    d.mu_x, d.mu_y, d.mu_dep = file_io.read_transport_coefficients(names, "mobility", model)
    d.D_x, d.D_y, d.D_dep = file_io.read_transport_coefficients(names, "Diffusion", model)
    d.k_dep = file_io.read_dependences(kfiles)
    d.k_x, d.k_y = file_io.read_rate_coefficients(kfiles, d.k_dep)
    d.De_diff = np.gradient(d.D_y[ns - 1], d.D_x[ns - 1]) / d.N0
    d.mue_diff = np.gradient(d.mu_y[ns - 1], d.mu_x[ns - 1]) / d.N0
    d.k_diff = [np.gradient(ky, kx) if dep == "Umean" else 0.0 for kx, ky, dep in zip(d.k_x, d.k_y, d.k_dep)]
    ns, n_eq, species, M, sign = ff.modify_approximation_vars("LMEA", ns, species, M, sign)
    d.ns, d.nr, d.n_eq = ns, len(kfiles), n_eq
    return d


def deck_programs(d):
    """``(tables, programs)`` of the script's refresh for a deck ``d`` (:func:`read_deck`, or a ``Case``): one
    program per field row, in the row order of FEDM_GD_N_FIELDS."""
    arg = {"Umean": "energy", "E/N": "redfield"}
    tables, progs = [], []

    def table(x, y):
        tables.append((np.asarray(x, dtype=float), np.asarray(y, dtype=float)))
        return len(tables) - 1

    e = d.ns - 1                                                                 # the electrons come last
    for dep, x, y in zip(d.mu_dep, d.mu_x, d.mu_y):                              # mobilities: N0 mu is tabulated
        progs.append(dict(kind="table", table=table(x, y), arg=arg[dep], scale=1.0 / d.N0) if dep in arg
                     else dict(kind="keep"))
    for i, (dep, x, y) in enumerate(zip(d.D_dep, d.D_x, d.D_y)):                 # diffusion coefficients
        progs.append(dict(kind="table", table=table(x, y), arg=arg[dep], scale=1.0 / d.N0) if dep in arg
                     else dict(kind="scaled_row", src_row=i, scale=kB * d.Tgas / elementary_charge) if dep == "ESR"
                     else dict(kind="keep"))
    for deriv, xs in ((d.mue_diff, d.mu_x), (d.De_diff, d.D_x)):                 # d mu_e / d eps, d D_e / d eps
        progs += [dict(kind="keep")] * e + [dict(kind="table", table=table(xs[e], deriv), arg="energy")]
    for dep, x, y in zip(d.k_dep, d.k_x, d.k_y):                                 # rate coefficients
        progs.append(dict(kind="table", table=table(x, y), arg=arg[dep]) if dep in arg else dict(kind="keep"))
    for dep, x, dy in zip(d.k_dep, d.k_x, d.k_diff):                             # ... and their energy derivatives
        progs.append(dict(kind="table", table=table(x, dy), arg="energy") if dep == "Umean" else dict(kind="keep"))
    return tables, progs + [dict(kind="me_old"), dict(kind="me"), dict(kind="ue_old")]


def same_programs(a, b):
    """Two (tables, programs) pairs describe the same refresh."""
    (ta, pa), (tb, pb) = a, b
    norm = lambda p: (p["kind"], p.get("table", 0) if p["kind"] == "table" else 0,
                      p.get("arg", "energy") if p["kind"] == "table" else "",
                      p.get("src_row", 0) if p["kind"] == "scaled_row" else 0,
                      p.get("scale", 1.0) if p["kind"] in ("table", "scaled_row") else 1.0)
    return len(ta) == len(tb) and all(np.array_equal(x, u) and np.array_equal(y, v) for (x, y), (u, v) in zip(ta, tb)) \
        and [norm(p) for p in pa] == [norm(p) for p in pb]


# ---- the meshes and potentials the tests share --------------------------------------------------------------------
GAP = 0.01


def crossed(nx, ny):
    from oracle.mesh import rectangle_crossed
    return rectangle_crossed(0.0, 0.0, GAP, GAP, nx, ny)


def refined():
    """The locally refined Delaunay mesh of tests/test_gpu_unstructured.py::test_lmea_kernels_on_an_unstructured_mesh."""
    from fedm_amd import meshgen
    size = meshgen.box_distance_size((0.0, 0.01, 0.0, 0.0015), 1.0e-4, 0.3, 1.2e-3)
    return meshgen.refined_rectangle(0.01, 0.01, size, 1.0e-4, n_levels=5)


def potential(coords, which, seed=0, fall=2e-4):
    """'ramp': the potential of the assembly tests, a linear drop of 100 V with 3 V of noise.  'steep': a cathode fall,
    -250 exp(-z / fall) with the same noise -- its consistent projection overshoots below zero behind the fall; with
    fall = 5e-5 it also passes the last knot of the E/N tables in front of it."""
    z = np.asarray(coords)[:, 1]
    noise = np.random.default_rng(seed).normal(0.0, 3.0, z.size)
    if which == "ramp":
        return -100.0 * (1.0 - z / GAP) + noise
    if which == "steep":
        return -250.0 * np.exp(-z / fall) + noise
    raise ValueError(which)
