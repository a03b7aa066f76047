"""The segregated (uncoupled) time step, no GPU: the binding, the facade, and what the float64 restatement
(tests/segregated_reference.py) says about the step on the numpy oracle.

Bounds used here and where they come from:

* residual rows after one restated step: each stage is a direct solve (the potential rows are linear; the species
  Newton stops at rtol 1e-10), so the rows it solved vanish to the Newton tolerance -- ``1e-8 |F rows before|``
  leaves two decades above the tolerance asked for;
* order: the splitting error is first order in dt, the ratio of the differences to the coupled run at dt and dt / 2
  is 2 in theory and 1.98-2.00 on the oracle; the interval [1.8, 2.2] is the issue's;
* planted faults: the GPU suite holds the device to the restatement within 1e-9 (tests/test_gpu_segregated.py);
  a fault must miss that by more than 100x, i.e. differ from the restatement by more than 1e-7.  The faults are
  O(dt / tau) effects, tau = eps0 / (e mu_e n_e) the dielectric relaxation time: in the run's initial state
  (n_e = 1e13 m^-3) tau is 1e5 steps and 20 faulty steps differ from the restatement by 4e-9 only.  They are
  therefore planted on that state with the electron density raised to 1e16 m^-3 (still four decades below a streamer
  head) and its potential made consistent, three steps (the stale field cannot show in a first step, whose starting
  field IS the consistent one).
"""
import ctypes as C
import re
import warnings
from pathlib import Path

import numpy as np
import pytest

import segregated_reference as sr

ROOT = Path(__file__).resolve().parent.parent
DEVICE_STATE_BOUND = 1e-9          # tests/test_gpu_segregated.py: device state against the restatement
N = 16                             # cells per side: the file stays well under a minute


# ---- the binding ---------------------------------------------------------------------------------------------------
def test_abi_version_and_the_new_entry_points():
    import __graft_entry__ as entry
    entry.build()
    from fedm_amd import _lib
    header = (ROOT / "include" / "fedm_hip.h").read_text()
    lib = _lib.load()
    assert lib.fedm_abi_version() == int(re.search(r"#define FEDM_ABI_VERSION (\d+)", header).group(1)) \
        == _lib.ABI_VERSION == 10
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int fedm_poisson_update(fedm_ctx *ctx, double rtol, int max_it, int *iterations);" in flat
    assert ("int fedm_newton_solve_species(fedm_ctx *ctx, const fedm_newton_opts *opts, fedm_newton_report *rep);"
            in flat)
    assert "int fedm_segregated_stats(fedm_ctx *ctx, int64_t out[8], int reset);" in flat
    # each cites the reference lines it replaces, and the timing kinds are documented
    assert "fedm/functions.py:1154-1161" in header and "fedm/functions.py:777-843" in header
    assert re.search(r"6 = species-only", header) and re.search(r"7 = the right-hand-side assembly", header)
    sig = dict(_lib._SIGNATURES)
    assert sig["fedm_poisson_update"] == sig["fedm_poisson_solve"]
    assert sig["fedm_newton_solve_species"] == sig["fedm_newton_solve"]
    res, args = sig["fedm_segregated_stats"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1] is C.POINTER(C.c_int64) and args[2] is C.c_int
    assert "int fedm_debug_species_linear_solve(fedm_ctx *ctx, const double *b, const fedm_newton_opts *opts, " \
           "double *x, int *its, double *rnorm);" in flat
    assert sig["fedm_debug_species_linear_solve"] == sig["fedm_debug_linear_solve"]
    assert "int fedm_debug_species_assembly(fedm_ctx *ctx, int jacobian);" in flat
    assert "int fedm_debug_block_product(fedm_ctx *ctx, int which, const double *x, double *y);" in flat
    for name in ("fedm_poisson_update", "fedm_newton_solve_species", "fedm_segregated_stats",
                 "fedm_debug_species_linear_solve", "fedm_debug_species_assembly", "fedm_debug_block_product"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == sig[name][1]
        assert name in _lib.exported_symbols()


# ---- the facade ----------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands where a device problem stands in PETScSNESSolver.solve."""

    def __init__(self):
        self.calls, self.mode = [], 0

    def krylov_scaling_mode(self):
        return self.mode

    def set_krylov_scaling(self, mode):
        self.mode = ("none", "rows").index(mode)

    def newton_solve(self, **kw):
        self.calls.append(("coupled", kw))
        return 1, True

    def segregated_solve(self, **kw):
        self.calls.append(("uncoupled", kw))
        return 1, True


class _Problem:
    before_solve = None

    def __init__(self):
        self.device = _Recorder()


def test_facade_coupling_parameter():
    from fedm_amd.device import DeviceProblem
    from fedm_amd.functions import PETScSNESSolver
    for name in ("poisson_update", "newton_solve_species", "segregated_solve", "segregated_stats"):
        assert callable(getattr(DeviceProblem, name))
    s = PETScSNESSolver()
    assert s.parameters["coupling"] == "coupled"
    assert s.parameters["poisson_relative_tolerance"] == 1e-10
    p = _Problem()
    s.solve(p)
    assert [c[0] for c in p.device.calls] == ["coupled"]           # the default is today's path
    s.parameters["coupling"] = "uncoupled"
    s.parameters["poisson_relative_tolerance"] = 1e-12
    s.parameters["relative_tolerance"] = 1e-7
    s.solve(p)
    kind, kw = p.device.calls[-1]
    assert kind == "uncoupled" and kw["poisson_rtol"] == 1e-12 and kw["rtol"] == 1e-7
    assert kw["ksp_rtol"] == s.parameters["krylov_relative_tolerance"]
    s.parameters["coupling"] = "segregated"
    with pytest.raises(ValueError, match="coupling"):
        s.solve(p)
    s.parameters["coupling"] = "uncoupled"
    s.parameters["krylov_residual_scaling"] = "rows"
    n_calls = len(p.device.calls)
    with pytest.raises(ValueError, match="rows"):
        s.solve(p)
    assert len(p.device.calls) == n_calls and p.device.mode == 0    # refused before anything was set or solved


def test_stepper_and_example_take_the_parameter():
    import inspect
    from fedm_amd.cases import streamer
    assert inspect.signature(streamer.Stepper.__init__).parameters["coupling"].default == "coupled"
    text = (ROOT / "examples" / "streamer_discharge.py").read_text()
    assert '"--coupling"' in text and 'newton.parameters["coupling"] = coupling' in text


def test_poisson_solver_goes_to_the_device_for_a_bound_form():
    from fedm_amd.functions import Poisson_solver

    class Dev:
        updates = 0

        def poisson_update(self):
            self.updates += 1

    class Bound:
        device = Dev()

    marker = object()
    assert Poisson_solver(None, Bound(), marker, [], None) is marker
    assert Bound.device.updates == 1


# ---- the restatement -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_case():
    from oracle import streamer as ost
    from oracle.mesh import rectangle_right
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, N, N)
    model = ost.build(mesh)
    return model, ost.initial_state(model)


def test_block_helpers_on_a_plain_matrix():
    import scipy.sparse as sp
    n_eq, nv = 3, 5
    J = sp.csr_matrix(np.arange(1.0, (n_eq * nv) ** 2 + 1).reshape(n_eq * nv, n_eq * nv))
    iu, ip = sr.block_indices(n_eq * nv, n_eq)
    assert list(ip) == [2, 5, 8, 11, 14] and len(iu) == 10 and not set(iu) & set(ip)
    assert np.array_equal(sr.species_block(J, n_eq).toarray(), J.toarray()[np.ix_(iu, iu)])
    assert np.array_equal(sr.potential_block(J, n_eq).toarray(), J.toarray()[np.ix_(ip, ip)])


def test_each_stage_solves_its_own_rows(oracle_case):
    model, U0 = oracle_case
    dt, dt_old = 5e-12, 1e30
    iu, ip = sr.block_indices(U0.size, 3)
    U = U0.copy()
    U[:, 2] *= 1.0 + 1e-3 * np.cos(7.0 * model.mesh.coords[:, 1] / model.mesh.coords[:, 1].max())   # an inconsistent field
    F_before, _ = model.residual_jacobian(U, U0, U0, dt, dt_old)
    sr.potential_stage(model, U, U0, U0, dt, dt_old)
    assert np.array_equal(U[:, :2], U0[:, :2])                      # the species entries are frozen
    F_mid, _ = model.residual_jacobian(U, U0, U0, dt, dt_old)       # densities still the OLD ones
    print(f"[segregated] potential rows {np.linalg.norm(F_before[ip]):.3e} -> {np.linalg.norm(F_mid[ip]):.3e}")
    assert np.linalg.norm(F_mid[ip]) <= 1e-8 * np.linalg.norm(F_before[ip])
    phi = U[:, 2].copy()
    rep = {}
    its = sr.species_stage(model, U, U0, U0, dt, dt_old, rtol=1e-10, report=rep)
    assert np.array_equal(U[:, 2], phi)                             # the potential entries are frozen, bit for bit
    F_end, _ = model.residual_jacobian(U, U0, U0, dt, dt_old)
    print(f"[segregated] species rows {rep['residual_history'][0]:.3e} -> {np.linalg.norm(F_end[iu]):.3e} in {its}")
    assert np.linalg.norm(F_end[iu]) <= 1e-8 * rep["residual_history"][0]
    # the potential rows no longer vanish for the NEW densities: that is the splitting error, not a mistake
    assert np.linalg.norm(F_end[ip]) > 10.0 * np.linalg.norm(F_mid[ip])


def test_first_order_against_the_coupled_run():
    from oracle import streamer as ost
    from oracle.newton import newton_solve

    def coupled(model, Uw, Uo, Uo1, dt, dto):
        newton_solve(model, Uw, Uo, Uo1, dt, dto, 1e-8, 20)

    diff = {}
    for dt in (5e-12, 2.5e-12):
        kw = dict(n=N, T_final=1e-10, dt_init=dt, dt_max=dt, ttol=1e3)
        Uc = ost.run(solver=coupled, **kw)[0]
        counts = []
        Us, _, t, _ = ost.run(solver=sr.solver(counts=counts, rtol=1e-8), **kw)
        assert len(counts) == round(1e-10 / dt) and abs(t - 1e-10) < 1e-16
        diff[dt] = sr.relative_difference(Us, Uc)
        print(f"[segregated] dt {dt:.2e}: {len(counts)} steps, species Newton its {sorted(set(counts))}, "
              f"difference to the coupled run {diff[dt]}")
    ratio = diff[5e-12] / diff[2.5e-12]
    print(f"[segregated] ratio {ratio}")
    assert np.all(diff[5e-12] < 1e-6)                                # small: the restatement is a sound yardstick
    assert np.all(ratio >= 1.8) and np.all(ratio <= 2.2)


def _three_steps(model, base, fault):
    U, Uo, Uo1 = base.copy(), base.copy(), base.copy()
    dt_old = 1e30
    for _ in range(3):
        Uo1[:] = Uo
        Uo[:] = U
        sr.segregated_step(model, U, Uo, Uo1, 5e-12, dt_old, fault=fault, rtol=1e-8)
        dt_old = 5e-12
    return U


@pytest.mark.parametrize("fault", ["swapped", "unfrozen", "stale"])
def test_planted_faults_miss_the_device_bound(oracle_case, fault):
    model, U0 = oracle_case
    base = U0.copy()
    base[:, 1] += np.log(1e3)                                       # n_e = 1e16 m^-3 (module docstring)
    sr.potential_stage(model, base, base, base, 5e-12, 1e30)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        right = _three_steps(model, base, None)
        wrong = _three_steps(model, base, fault)
    d = sr.relative_difference(wrong, right)
    print(f"[segregated] fault {fault}: difference to the restatement {d}")
    assert d.max() > 100.0 * DEVICE_STATE_BOUND


def test_unknown_fault_is_refused(oracle_case):
    model, U0 = oracle_case
    with pytest.raises(ValueError):
        sr.segregated_step(model, U0.copy(), U0, U0, 5e-12, 1e30, fault="other")
