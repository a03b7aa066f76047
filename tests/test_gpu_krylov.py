"""The GMRES driver and the Newton loop of fedm_amd/csrc/krylov.cpp and newton.cpp against float64, path by path.

What the solvers are fed is pinned elsewhere (assembly, the preconditioner, J x).  Here: what they do with it.  Every
linear case solves ``J x = b`` through ``DeviceProblem.linear_solve`` (``fedm_debug_linear_solve``: the very ``gmres()``
call the Newton loop makes) with ``J = jacobian_csr()`` and asserts, with every norm taken in float64 on the host:

1. ``true = |J x - b|`` against ``tol = max(ksp_rtol |b|, ksp_atol)``: ``true <= tol (1 + g)`` when the solver
   returns 0 (preconditioner on the left: the same on ``M^-1 (J x - b)``, M^-1 from ``fieldsplit_apply``, or the
   inverse of the diagonal blocks formed in numpy when there is no hierarchy);
2. ``|true - reported| / |b|``, the drift of the recurrence (zero in exact arithmetic);
3. the returned step count equals the counters' used steps (launched - dropped) and is ``<= ksp_max_it``;
4. the path counters (``fedm_solver_path_stats``) show the path the case is for.

Two conditions are fixed and are no measurements: ``true <= 2 tol`` at ``ksp_rtol = 1e-5`` (what every script and the
bench use) and ``true <= 10 tol`` at ``1e-10``.  The figures ``g`` (= true / tol - 1, where positive) and the drift are
measured against the float64 residual and bounded at 10x the worst value of their family (MEASURED below).  Since a
solve that returns 0 has had its true residual checked on the device, assertion 1 reads
``true <= tol (1 + g) + drift bound * |b|`` with g = 0.

The Newton loop is followed on the device's own J and F: one iteration against its linear system, ``stol`` / ``atol``,
the iteration hint and the cached error norm, each with its counters.

Switches the library reads once per process run in child processes of their own (``python tests/test_gpu_krylov.py``).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent

pytestmark = pytest.mark.gpu

LINEAR, NAN = 3, 2            # FEDM_DIVERGED_LINEAR, FEDM_DIVERGED_NAN

# Measured on an MI355X, 2026-10-16, every solve of this file against its float64 residual (each test prints its figures
# before it asserts; six runs).  Per family: the worst `true / tol - 1` of the solves that returned 0 and the worst drift
# `|true - reported| / |b|`.
#
#   family                                         worst true/tol - 1      worst drift
#   right, as found (recurrence's norm reported)   +2.39 (11 steps, 1e-7)  2.7e-7   <- the fault fixed here
#   left,  as found (M^-1 b - M^-1 J x at restarts) +4007 (init48, 1e-10)   4.0e-7   <- the fault fixed here
#   right, true residual checked                   < 0 (0.98 tol at most)  2.7e-15
#   left,  true residual checked (field split)     < 0 (0.98 tol at most)  1.0e-14  (2.5e-16 .. 1.0e-14 over the runs)
#   jacobi (point-block Jacobi on the left)        < 0 (0.998 tol)         2.8e-11
#
# Per case (first solve / solve with the hint; true / tol and drift), run of 2026-10-16 with the fixes in:
#   short-init48 0.0028 7e-18 | short-graded-init 0.0069 6e-19 | short-head48-1e-4 0.50 6e-17 | boundary-head48-1e-5
#   0.74 1e-15 | long-head48-1e-6 0.34 1e-15 | long-head48-3e-7 2e-6 7e-16 | long-head48-1e-7 6e-6 2e-16 |
#   long-head48-1e-10 0.0035 3e-17 | long-refined-1e-10 0.31 9e-16 | four-species 0.30 3e-18 | four-species-1e-10 1e-5
#   4e-18 | glow-discharge 0.45 3e-16 | random-head48 0.86 3e-18 | restarts m = 3, 5, 8: 0.23, 0.49, 0.80, 7e-16 |
#   left 1e-5 / 1e-6 / 1e-10: init48 0.62 0.58 0.47, head48 0.98 0.63 0.70, four 0.77 0.25 0.22, drift <= 1.0e-14.
#
# As found, a solve of more than a few steps reported the recurrence's norm, which one-pass Gram-Schmidt lets drift: 5x
# below the true residual after 11 steps (head48, ksp_rtol 1e-7: true = 3.4 tol with return code 0), and on the
# Dirichlet-row right-hand side true = 2.2 tol at ksp_rtol 1e-5, which misses the fixed condition.  On the left the
# restarts formed M^-1 b - M^-1 J x, two vectors rounded to single precision inside M^-1: code 0 at 1e-10 with
# M^-1 (J x - b) at 4.7, 9.3 and 4008 times the tolerance.  Now every field-split solve that ends on the generic update
# forms the true residual (on the left: M^-1 of the double-precision b - J x) before it reports success, so no such
# solve returns 0 above its tolerance: g = 0, and the bound on the true residual is tol + DRIFT_BOUND |b| (the device's
# float64 norm against the host's).
MEASURED = {
    # family: (worst true / tol - 1 [negative: below the tolerance], worst drift)
    "right": (-0.02, 2.7e-15),
    "left": (-0.02, 1.0e-14),
    "jacobi": (-0.002, 2.8e-11),
}
G_BOUND = {"right": 0.0, "left": 0.0, "jacobi": 0.0}
DRIFT_BOUND = {family: 10.0 * drift for family, (_, drift) in MEASURED.items()}
FIXED = {1e-5: 2.0, 1e-10: 10.0}      # true <= FIXED[ksp_rtol] * tol: set in advance, not measured


# ---- contexts ------------------------------------------------------------------------------------------------------
def _streamer48(state):
    """The streamer model on ``streamer.mesh(48, 4.0)``: its initial state ("init": the early streamer, 2-3 Krylov
    steps a solve) or a developed head ("head"), with the V(1,1) cycle and the degree-6 species polynomial."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    msh = streamer.mesh(48, 4.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    if state == "init":
        U = np.zeros((prob.nv, 3))
        U[:, 0], U[:, 1] = streamer.initial_log_densities(prob.coords)
        prob.set_state(U, U, U)
        prob.set_step(5e-12, 1e30)
    else:
        from test_gpu_preconditioner import _head_state
        _head_state(prob, prob.coords)
    prob.setup_multigrid(nu=1, omega=0.85, max_coarse=40)
    prob.set_fieldsplit(chebyshev_weights(6))
    if state == "init":
        prob.poisson_solve(rtol=1e-12)
        U = prob.get_state()
        prob.set_state(U, U, U)
    return prob


def make_problem(name):
    """A context with its Jacobian assembled: (problem, J in the caller's numbering, F of that assembly)."""
    if name in ("init48", "head48"):
        prob = _streamer48(name[:4])
    else:
        import test_gpu_preconditioner as tp
        prob = tp.build({"four": "four-species", "glow": "glow-discharge", "refined": "refined-head",
                         "graded-init": "graded-init"}[name])[0]
    prob.jacobian()
    return prob, prob.jacobian_csr(), prob.residual_vector()


def rhs_of(kind, prob, J, F):
    if kind == "residual":
        return -F
    rng = np.random.default_rng(11)
    if kind == "random":                     # b = J x: every block of J leaves its mark
        from fieldsplit_reference import balanced_rhs
        return balanced_rhs(J, prob.n_eq - 1, rng)
    if kind == "dirichlet":                  # supported on the Dirichlet rows (identity rows of J)
        from fedm_amd.cases import streamer
        b = np.zeros(prob.n)
        rows = np.asarray(streamer.dirichlet(prob.coords)[0])
        b[rows] = rng.standard_normal(rows.size)
        return b
    raise KeyError(kind)


# ---- one solve, measured -------------------------------------------------------------------------------------------
def _minv(prob, J, side_left, hierarchy):
    """M^-1 of the left-preconditioned system as a function of a vector in the caller's numbering."""
    if not side_left and hierarchy:
        return None
    if hierarchy:
        return lambda v: prob._back(prob.fieldsplit_apply(prob._vec(v)))
    from krylov_reference import block_jacobi
    return block_jacobi(J, prob.n_eq)


def solve_and_measure(prob, J, b, left=False, hierarchy=True, **ksp):
    """One ``linear_solve`` and its figures: float64 residual of the system the side in use tests, the tolerance, the
    reported norm, the counters of this solve alone."""
    ksp = {**dict(ksp_restart=30, ksp_rtol=1e-5, ksp_atol=1e-50, ksp_max_it=10000), **ksp}
    prob.solver_path_stats(reset=True)
    x, its, rnorm, code = prob.linear_solve(b, **ksp)
    stats = prob.solver_path_stats(reset=True)
    minv = _minv(prob, J, left, hierarchy)         # (after the counters are read: it launches nothing they count)
    r = J @ x - b
    bb = b
    if minv is not None:
        r, bb = minv(r), minv(b)
    true, bnorm = float(np.linalg.norm(r)), float(np.linalg.norm(bb))
    tol = max(ksp["ksp_rtol"] * bnorm, ksp["ksp_atol"])
    return dict(x=x, its=its, rnorm=rnorm, code=code, true=true, bnorm=bnorm, tol=tol, stats=stats,
                ratio=true / tol if tol > 0 else float("inf"), drift=abs(true - rnorm) / bnorm if bnorm > 0 else 0.0,
                ksp=ksp, family="right" if minv is None else ("left" if hierarchy else "jacobi"))


def _show(label, m):
    s = {k: v for k, v in m["stats"].items() if v}
    print(f"[krylov] {label}: code {m['code']} its {m['its']} reported {m['rnorm']:.6e} true {m['true']:.6e} "
          f"tol {m['tol']:.6e} true/tol {m['ratio']:.4f} drift {m['drift']:.3e} |b| {m['bnorm']:.3e} {s}", flush=True)


def check(label, m, expect_code=0, residual_floor=0.0):
    """Assertions 1-3 on one measured solve.  ``residual_floor``: what the evaluation of the residual itself may differ
    by between the device and the host (an absolute norm; for right-hand sides far below |J| |x|)."""
    _show(label, m)
    s = m["stats"]
    assert m["code"] == expect_code
    assert np.isfinite(m["x"]).all()
    assert m["its"] == s["steps_used"] == s["steps_single"] + s["steps_pair"] + s["steps_last"] - s["steps_dropped"]
    assert m["its"] <= m["ksp"]["ksp_max_it"]
    if m["family"] == "left":
        # both norms pass through M^-1, which rounds to single precision inside and sums in an order that is not fixed:
        # the device's M^-1 r and the host's (the same kernels, another run) differ by up to eps32 |M^-1 r| each
        residual_floor += 2.0 * float(np.finfo(np.float32).eps) * m["true"]
    assert m["drift"] * m["bnorm"] <= DRIFT_BOUND[m["family"]] * m["bnorm"] + residual_floor, (m["drift"], residual_floor)
    if expect_code == 0:
        assert m["true"] <= m["tol"] * (1.0 + G_BOUND[m["family"]]) + DRIFT_BOUND[m["family"]] * m["bnorm"]
        for rtol, factor in FIXED.items():
            if m["ksp"]["ksp_rtol"] == rtol:
                assert m["true"] <= factor * m["tol"]
    else:
        assert m["true"] > m["tol"]           # the failure reported is a real one


# ---- the table -----------------------------------------------------------------------------------------------------
# id: context, right-hand side, solver options, the band the step count must lie in.  The bands' inputs were chosen with
# the float64 restatement's count and the device's own first measurement (2026-10-16): init48 3 steps at 1e-5, 6 at
# 1e-10; head48 8 at 1e-4, 9 at 1e-5, 11 at 1e-6, 30-38 at 1e-10 (not reproducible from run to run there: the
# assembly's atomics order the sums differently and near the floor of the arithmetic a step more or less decides).
CASES = {
    "short-init48": dict(problem="init48", its=(1, 8)),
    "short-graded-init": dict(problem="graded-init", its=(1, 8)),
    "short-head48-1e-4": dict(problem="head48", ksp=dict(ksp_rtol=1e-4), its=(1, 8)),
    "boundary-head48-1e-5": dict(problem="head48", its=(9, 30)),
    "long-head48-1e-6": dict(problem="head48", ksp=dict(ksp_rtol=1e-6), its=(9, 30)),
    "long-head48-3e-7": dict(problem="head48", ksp=dict(ksp_rtol=3e-7), its=(9, 30)),
    "long-head48-1e-7": dict(problem="head48", ksp=dict(ksp_rtol=1e-7), its=(9, 60)),
    "long-head48-1e-10": dict(problem="head48", ksp=dict(ksp_rtol=1e-10), its=(9, 90)),
    "long-refined-1e-10": dict(problem="refined", ksp=dict(ksp_rtol=1e-10), its=(9, 90)),
    "four-species": dict(problem="four", its=(1, 8)),
    "four-species-1e-10": dict(problem="four", ksp=dict(ksp_rtol=1e-10), its=(9, 90)),
    "glow-discharge": dict(problem="glow", left=True, its=(1, 30)),
    "random-head48": dict(problem="head48", rhs="random", its=(1, 8)),
}


@pytest.mark.parametrize("case_id", sorted(CASES))
def test_one_solve(case_id):
    case = CASES[case_id]
    prob, J, F = make_problem(case["problem"])
    b = rhs_of(case.get("rhs", "residual"), prob, J, F)
    left = case.get("left", False)
    first = solve_and_measure(prob, J, b, left=left, **case.get("ksp", {}))
    check(case_id + " (first solve: no hint)", first)
    again = solve_and_measure(prob, J, b, left=left, **case.get("ksp", {}))   # with the hint of the solve before
    check(case_id + " (hint = its)", again)
    prob.close()
    lo, hi = case["its"]
    for m in (first, again):
        assert lo <= m["its"] <= hi
        s = m["stats"]
        assert s["cycles"] >= 1 and s["generic_updates"] == s["cycles"] and s["fused_updates"] == 0 and s["solves"] == 1
        assert s["deferred_norm"] == (1 if left else 0)
        if not left:           # (the left cases have a test of their own)
            assert s["verified"] >= 1
            if hi <= 30:
                assert s["cycles"] == 1 + s["verify_failed"] and s["verified"] == s["cycles"]
    assert first["stats"]["steps_ahead"] == 0          # no hint yet: nothing is launched ahead
    if not left and again["its"] > 1:
        assert again["stats"]["steps_ahead"] >= 1
    if case.get("ksp", {}).get("ksp_rtol", 1e-5) >= 1e-6:
        assert again["its"] == first["its"]


@pytest.mark.parametrize("restart", [3, 5, 8])
def test_restart_on_one_gpu(restart):
    """Finding: steps are launched ahead in every cycle, not in cycle 0 only (`wanted()` compares the index inside the
    cycle with the whole previous solve's count); they write vectors nobody reads, and assertion 1 holds."""
    prob, J, F = make_problem("head48")
    ksp = dict(ksp_rtol=1e-6)
    full = solve_and_measure(prob, J, -F, **ksp)
    check("restart reference m=30", full)
    assert full["its"] >= 10
    m = solve_and_measure(prob, J, -F, ksp_restart=restart, **ksp)
    check(f"restart m={restart}", m)
    prob.close()
    s = m["stats"]
    assert s["cycles"] >= 2 and s["generic_updates"] == s["cycles"] and s["steps_ahead"] >= 1
    assert s["verified"] == s["cycles"]
    assert m["its"] > restart


@pytest.mark.parametrize("problem,restart", [("init48", 1), ("head48", 30)])
def test_restart_without_a_hierarchy(problem, restart):
    """Point-block Jacobi on the left (no hierarchy): tens to hundreds of steps, many cycles."""
    prob, J, F = make_problem(problem)
    prob.clear_multigrid()
    m = solve_and_measure(prob, J, -F, left=True, hierarchy=False, ksp_restart=restart, ksp_max_it=2000)
    check(f"block Jacobi {problem} m={restart}", m)
    prob.close()
    assert m["stats"]["cycles"] >= 2 and m["stats"]["deferred_norm"] == 1 and m["its"] > 30


def test_hint_too_short_and_too_long():
    prob, J, F = make_problem("init48")
    short = dict(ksp_rtol=1e-5)
    long_ = dict(ksp_rtol=1e-10)
    a = solve_and_measure(prob, J, -F, **short)
    check("short solve", a)
    a = solve_and_measure(prob, J, -F, **short)        # the hint is now this solve's own count
    check("short solve again", a)
    assert 1 <= a["its"] <= 4
    assert a["stats"]["steps_last"] >= 1               # the expected last step went in without its update
    b = solve_and_measure(prob, J, -F, **long_)
    check("long solve after a short one", b)
    assert b["its"] >= a["its"] + 2
    assert b["stats"]["updates_made_up"] >= 1
    c = solve_and_measure(prob, J, -F, **short)
    check("short solve after a long one", c)
    assert c["stats"]["steps_dropped"] >= 1 and c["its"] == a["its"]
    d = solve_and_measure(prob, J, -F, **long_)         # unread publications must not leak into the next solve
    check("long solve after the dropped steps", d)
    prob.close()
    assert np.linalg.norm(J @ (d["x"] - b["x"])) <= 2.0 * b["tol"] * (1.0 + G_BOUND["right"])


def test_nothing_to_solve():
    prob, J, F = make_problem("init48")
    for label, b, ksp in (("b = 0", np.zeros(prob.n), {}),
                          ("|b| <= atol", 1e-3 * F / np.linalg.norm(F), dict(ksp_atol=2e-3))):
        for left in (False, True):
            prob.set_preconditioner_side("left" if left else "right")
            prob.jacobian()
            prob.solver_path_stats(reset=True)
            x, its, rnorm, code = prob.linear_solve(b, **ksp)
            s = prob.solver_path_stats(reset=True)
            print(f"[krylov] nothing to solve, {label}, left={left}: code {code} its {its} rnorm {rnorm} {s}", flush=True)
            assert code == 0 and its == 0 and s["steps_used"] == 0
            assert s["nothing_to_solve"] == 1 and s["deferred_norm"] == (1 if left else 0)
            assert np.array_equal(x, np.zeros(prob.n))
    prob.close()


def test_exhaustion():
    prob, J, F = make_problem("head48")
    full = solve_and_measure(prob, J, -F, ksp_rtol=1e-10)
    check("exhaustion reference", full)
    assert full["its"] >= 10
    m = solve_and_measure(prob, J, -F, ksp_rtol=1e-10, ksp_max_it=3)
    check("max_it=3", m, expect_code=LINEAR)
    assert m["its"] == 3 and m["stats"]["exhausted"] == 1 and m["stats"]["cycles"] == 1
    m = solve_and_measure(prob, J, -F, ksp_rtol=1e-10, ksp_restart=5, ksp_max_it=7)
    check("max_it=7 inside the second cycle", m, expect_code=LINEAR)
    assert m["its"] == 7 and m["stats"]["exhausted"] == 1 and m["stats"]["cycles"] == 2
    # through the Newton loop: a RuntimeError, the state of the failed solve reported
    with pytest.raises(RuntimeError, match="linear"):
        prob.newton_solve(rtol=1e-8, ksp_rtol=1e-10, ksp_max_it=3)
    assert not prob.last_report.converged
    prob.close()


def _nan_run():
    prob, J, F = make_problem("init48")
    b = -F.copy()
    b[prob.n // 2] = np.nan
    rec = []
    for left in (False, True):
        prob.set_preconditioner_side("left" if left else "right")
        prob.jacobian()
        x, its, rnorm, code = prob.linear_solve(b)
        rec.append(dict(left=left, code=code, its=its))
    # the context is usable afterwards
    prob.set_preconditioner_side("right")
    prob.jacobian()
    m = solve_and_measure(prob, J, -F)
    check("after the NaN", m)
    prob.close()
    return rec + [dict(code=m["code"], its=m["its"])]


def test_adaptive_solver_retries_after_an_exhausted_linear_solve(tmp_path):
    """FEDM_DIVERGED_LINEAR -> RuntimeError -> adaptive_solver's catch-all halves the step and repeats it; the run goes
    on.  (The same road a solve takes that gives up because its true residual stays above the tolerance.)"""
    from fedm_amd.cases import streamer
    msh = streamer.mesh(32, 4.0)
    prob = streamer.device_problem(msh.coords, msh.cells)
    st = streamer.Stepper(prob, error_file=tmp_path / "relative error.log")
    st.initialise()
    solve, calls = prob.newton_solve, []

    def limited(*a, **kw):                     # the first attempt of the step may take one Krylov step only
        calls.append(len(calls))
        if len(calls) == 1:
            kw["ksp_max_it"] = 1
        return solve(*a, **kw)
    prob.newton_solve = limited
    dt0 = st.dt.time_step
    prob.solver_path_stats(reset=True)
    st.step()
    s = prob.solver_path_stats()
    print(f"[krylov] retry: {len(calls)} attempts, dt {dt0} -> {st.dt_old.time_step}, {s}", flush=True)
    assert len(calls) >= 2 and s["exhausted"] == 1
    assert st.dt_old.time_step == pytest.approx(0.5 * dt0)        # the accepted step is the halved one
    assert prob.last_report.converged and np.all(np.isfinite(prob.get_state()))
    st.step()                                                      # ... and the run goes on
    assert st.steps == 2 and prob.last_report.converged
    prob.close()


def test_non_finite_right_hand_side():
    """One NaN in b: FEDM_DIVERGED_NAN on either side and a context that still solves -- one run, in a process of its own
    under its own time limit (a host poll that never saw its tag would otherwise hold the whole suite)."""
    rec = _child({}, "nan", timeout=120)
    print(f"[krylov] NaN in b: {rec}", flush=True)
    assert [(r["code"], r["its"]) for r in rec[:2]] == [(NAN, 0), (NAN, 0)]
    assert rec[2]["code"] == 0 and rec[2]["its"] >= 1


@pytest.mark.parametrize("problem", ["init48", "head48", "four"])
def test_left_preconditioning(problem):
    prob, J, F = make_problem(problem)
    prob.set_preconditioner_side("left")
    prob.jacobian()
    # (as found the device returned 0 at 1e-10 with M^-1 (J x - b) at 4.7, 9.3 and 4008 times the tolerance: its
    # restarts formed M^-1 b - M^-1 J x, two vectors rounded to single precision inside M^-1; they now form
    # M^-1 (b - J x) from the double-precision residual, and the solve is checked against it before it reports success)
    for rtol in (1e-5, 1e-6, 1e-10):
        m = solve_and_measure(prob, J, -F, left=True, ksp_rtol=rtol)
        check(f"left {problem} rtol={rtol}", m)
        assert m["stats"]["deferred_norm"] == 1 and m["stats"]["verified"] >= 1
        assert (m["stats"]["cycles"] == 1) == (m["stats"]["verify_failed"] == 0 and m["its"] <= 30)
        assert m["stats"]["steps_ahead"] == 0 and m["stats"]["steps_pair"] == 0
    prob.close()


def test_graphs_and_plain_launches_take_the_same_steps():
    prob, J, F = make_problem("head48")
    out = []
    for plain in (False, True):
        if plain:
            prob.profile(2)
        for ksp in (dict(), dict(ksp_rtol=1e-6), dict(ksp_rtol=1e-6, ksp_restart=5)):
            m = solve_and_measure(prob, J, -F, **ksp)
            check(f"plain={plain} {ksp}", m)
            out.append(m)
    prob.close()
    for g, p in zip(out[:3], out[3:]):
        assert g["its"] == p["its"] and g["stats"]["cycles"] == p["stats"]["cycles"]
        assert p["stats"]["steps_pair"] == 0
        assert np.linalg.norm(J @ (g["x"] - p["x"])) <= 2.0 * g["tol"] * (1.0 + G_BOUND["right"])


# (the side last: every other setter is followed on the right, where the captured steps go in pairs and ahead)
SETTERS = ("weights", "order", "hierarchy", "assembly", "side")


def _apply_setting(prob, setting):
    from fedm_amd.device import chebyshev_weights
    if setting == "weights":
        prob.set_fieldsplit(chebyshev_weights(4))
    elif setting == "order":
        prob.set_fieldsplit_order("upper")
    elif setting == "side":
        prob.set_preconditioner_side("left")
    elif setting == "hierarchy":
        prob.clear_multigrid()
        prob.setup_multigrid(nu=2, omega=0.67, max_coarse=40)
    elif setting == "assembly":
        prob.set_assembly("colour")


def test_setters_leave_no_stale_captured_steps():
    """On ONE context a solve, then each setter in turn and a solve: against a fresh context that had every setting up
    to that point from the start."""
    prob, J, F = make_problem("head48")
    ksp = dict(ksp_rtol=1e-5)
    check("before any setter", solve_and_measure(prob, J, -F, **ksp))
    left = False
    for i, setting in enumerate(SETTERS):
        _apply_setting(prob, setting)
        prob.jacobian()
        J1, F1 = prob.jacobian_csr(), prob.residual_vector()
        left = left or setting == "side"
        m = solve_and_measure(prob, J1, -F1, left=left, **ksp)
        check(f"after set {setting}", m)
        fresh, _, _ = make_problem("head48")
        for s in SETTERS[:i + 1]:
            _apply_setting(fresh, s)
        fresh.jacobian()
        f = solve_and_measure(fresh, fresh.jacobian_csr(), -fresh.residual_vector(), left=left, **ksp)
        check(f"fresh context with {SETTERS[:i + 1]}", f)
        fresh.close()
        assert m["its"] == f["its"]
        # both solve the same system (two assemblies differ in their last bits only) to the tolerance
        assert np.linalg.norm(J1 @ (m["x"] - f["x"])) <= 2.0 * np.linalg.norm(F1) * (1e-5 * (1.0 + G_BOUND["right"])
                                                                                    + DRIFT_BOUND["right"])
    prob.close()


def test_second_pass():
    """A right-hand side on one Dirichlet row (an identity row of J): the Krylov vectors all but repeat themselves and
    the second Gram-Schmidt pass runs.  (The happy breakdown h_{j+1,j} == 0 exactly was not reached with any input
    tried: on the device the norm never cancels to an exact zero.)"""
    from fedm_amd.cases import streamer
    prob, J, F = make_problem("init48")
    b = np.zeros(prob.n)
    b[np.asarray(streamer.dirichlet(prob.coords)[0])[3]] = 1.0
    m = solve_and_measure(prob, J, b)
    # |b| = 1 beside rows of J with entries of 1e15: the residual's own float64 evaluation carries a forward error of
    # (w + 2) eps | |J| |x| + |b| | (w entries a row), on the device and on the host alike: no drift of the recurrence
    width = int(np.diff(J.indptr).max())
    floor = 2.0 * (width + 2) * np.finfo(float).eps * float(np.linalg.norm(abs(J) @ np.abs(m["x"]) + np.abs(b)))
    check("one Dirichlet row", m, residual_floor=floor)
    prob.close()
    assert m["stats"]["second_passes"] >= 1 and m["stats"]["breakdowns"] == 0


def test_no_success_is_reported_above_the_tolerance():
    """The regression test of the fault found here: a random right-hand side on all Dirichlet rows, ksp_rtol 1e-5.  As
    found the solver returned 0 with true = 2.2 tol (the recurrence's norm had drifted: 2.9e-5 reported, 2.0e-4 true).
    The floor of the residual's own arithmetic (J has entries of 1e15 beside these rows) is about the tolerance here, so
    the solve may legitimately fail -- but it must say so: 0 only within the fixed 2 tol, FEDM_DIVERGED_LINEAR
    otherwise, with the norm it reports being the true one to the accuracy of that floor.  Measured (2026-10-16, three
    runs): FEDM_DIVERGED_LINEAR after 96-98 steps with true = 1.18-1.27 tol, three failed checks.  In a Newton solve that
    return becomes a RuntimeError, which adaptive_solver answers with a halved step
    (test_adaptive_solver_retries_after_an_exhausted_linear_solve); the Newton right-hand sides of this file all
    converge."""
    prob, J, F = make_problem("init48")
    b = rhs_of("dirichlet", prob, J, F)
    m = solve_and_measure(prob, J, b)
    _show("Dirichlet rows", m)
    prob.close()
    assert m["code"] in (0, LINEAR) and m["stats"]["verified"] >= 1
    if m["code"] == 0:
        assert m["true"] <= FIXED[1e-5] * m["tol"]
    else:
        assert m["stats"]["verify_failed"] >= 1 and m["rnorm"] > m["tol"]
        assert 0.5 * m["true"] <= m["rnorm"] <= 2.0 * m["true"]


# ---- the Newton loop ------------------------------------------------------------------------------------------------
def _start(prob, u0):
    prob.set_state(u0, u0, u0)
    prob.solver_path_stats(reset=True)


def _truncated(prob, u0, k):
    """The state after exactly k Newton updates from u0."""
    _start(prob, u0)
    with pytest.raises(RuntimeError, match="maximum"):
        prob.newton_solve(rtol=1e-30, atol=0.0, max_it=k)
    assert prob.last_report.iterations == k and not prob.last_report.converged
    return prob.get_state().copy()


# problem, ksp_rtol, the update that must run, the Krylov steps it must take (None: only the side of the boundary)
# (at 1e-8 and 1e-10 init48 takes 4-6 steps in most runs and ~30 in some -- near the floor of the arithmetic a step
# more or less decides --, so those cases assert the path they took against their step count only; 1e-7 is 3 steps)
NEWTON_ITERATIONS = [("init48", 1e-5, "fused_updates", None), ("init48", 1e-7, "fused_updates", None),
                     ("init48", 1e-8, None, None), ("init48", 1e-10, None, None),
                     ("head48", 1e-4, "fused_updates", 8), ("head48", 1e-5, "generic_updates", 9)]


@pytest.mark.parametrize("problem,ksp_rtol,path,steps", NEWTON_ITERATIONS)
def test_one_newton_iteration_solves_its_linear_system(problem, ksp_rtol, path, steps):
    """u1 - u0 of a single iteration against J(u0) delta = -F(u0) in float64: the fused update (what the bench and the
    scripts run: up to 8 steps in one cycle, the recurrence's norm trusted) at 1e-5, at 1e-10 and with all 8
    coefficients, the generic update right behind the boundary at 9.  The fixed conditions hold for the fused path as
    for any other: 2 tol at 1e-5 (and at the looser 1e-4), 10 tol at 1e-10 (and at 1e-8).  The assembly by global
    colouring is used: it is reproducible bit for bit, so J and F read here are the ones the iteration solved with (two
    patch assemblies differ by ~2e-9 |F|, the rounding floor of DESIGN.md section 4: ten times a 1e-10 tolerance)."""
    prob, _, _ = make_problem(problem)
    prob.set_assembly("colour")
    prob.jacobian()
    J, F = prob.jacobian_csr(), prob.residual_vector()
    prob.jacobian()
    assert np.array_equal(prob.residual_vector(), F)
    u0 = prob.get_state().copy()
    uo = prob.get_state_old().copy()
    prob.solver_path_stats(reset=True)
    with pytest.raises(RuntimeError, match="maximum"):
        prob.newton_solve(rtol=1e-30, atol=0.0, max_it=1, ksp_rtol=ksp_rtol)
    s = prob.solver_path_stats()
    delta = (prob.get_state() - u0).ravel()
    assert np.array_equal(prob.get_state_old(), uo)
    true, tol = float(np.linalg.norm(J @ delta + F)), ksp_rtol * float(np.linalg.norm(F))
    # delta is read as u1 - u0, and u1 = fl(u0 + delta) has lost what is below half an ulp of u1 (the potential is 1e4
    # beside updates of 1e-6): the residual of the delta so read differs from the solve's own by up to | |J| ulp(u1)/2 |
    rounding = float(np.linalg.norm(abs(J) @ (0.5 * np.finfo(float).eps * np.abs(prob.get_state().ravel()))))
    print(f"[krylov] one Newton iteration {problem} ksp_rtol {ksp_rtol}: true {true:.6e} tol {tol:.6e} "
          f"true/tol {true / tol:.4f} rounding of u1 {rounding:.3e} { {k: v for k, v in s.items() if v} }", flush=True)
    prob.close()
    assert true <= FIXED[1e-10 if ksp_rtol < 1e-5 else 1e-5] * tol + rounding
    assert s["fused_updates"] + s["generic_updates"] == s["cycles"] and s["solves"] == 1
    assert s["newton_max_it"] == 1
    assert prob.last_report.linear_iterations == s["steps_used"]
    assert (s["steps_used"] <= 8) == (s["fused_updates"] == 1)
    if path is not None:
        assert s[path] == 1 and s["cycles"] == 1
    if steps is not None:
        assert s["steps_used"] == steps


def test_stol_atol_and_the_iteration_hint():
    prob, J, F = make_problem("init48")
    u0 = prob.get_state().copy()
    u1, u2 = _truncated(prob, u0, 1), _truncated(prob, u0, 2)
    s2 = float(np.linalg.norm(u2 - u1) / np.linalg.norm(u2))          # |delta| / |u| of iteration 2, float64
    print(f"[krylov] stol: |delta_2| / |u_2| = {s2:.6e}", flush=True)
    for factor, its in ((1.01, 2), (0.99, 3)):
        _start(prob, u0)
        assert prob.newton_solve(rtol=1e-30, atol=0.0, stol=factor * s2, max_it=6)[0] == its
        assert prob.solver_path_stats()["fused_updates"] == its       # the norms came from the fused update's slots
    # the same through the generic update (a solve of more than 8 steps: ksp_rtol 1e-10 is 6 steps here, so by a restart)
    _start(prob, u0)
    with pytest.raises(RuntimeError, match="maximum"):
        prob.newton_solve(rtol=1e-30, atol=0.0, max_it=2, ksp_restart=2, ksp_rtol=1e-8)
    g1 = prob.get_state().copy()
    _start(prob, u0)
    with pytest.raises(RuntimeError, match="maximum"):
        prob.newton_solve(rtol=1e-30, atol=0.0, max_it=1, ksp_restart=2, ksp_rtol=1e-8)
    g0 = prob.get_state().copy()
    sg = float(np.linalg.norm(g1 - g0) / np.linalg.norm(g1))
    for factor, its in ((1.01, 2), (0.99, 3)):
        _start(prob, u0)
        assert prob.newton_solve(rtol=1e-30, atol=0.0, stol=factor * sg, max_it=6, ksp_restart=2, ksp_rtol=1e-8)[0] == its
        st = prob.solver_path_stats()
        assert st["generic_updates"] >= its and st["fused_updates"] <= 1
    # atol at iteration 0: a converged state is left untouched bit for bit
    _start(prob, u0)
    prob.newton_solve(rtol=1e-6)
    u = prob.get_state().copy()
    prob.solver_path_stats(reset=True)
    assert prob.newton_solve(rtol=1e-6, atol=10.0 * prob.last_report.fnorm)[0] == 0
    assert np.array_equal(prob.get_state(), u) and prob.solver_path_stats()["solves"] == 0
    prob.close()


def test_newton_loop_follows_the_reference_loop_on_the_device_systems():
    """The restated Newton loop (krylov_reference.newton, direct solves) fed with the DEVICE's F and J, taken out state
    by state: same number of iterations, same first residual norm, and -- the linear solves at 1e-10 -- the same
    sequence of residual norms to 1e-3 while the rounding floor of F (~2e-9 |F0|) is below that."""
    import krylov_reference as kr
    prob, _, _ = make_problem("init48")
    prob.set_assembly("colour")                       # reproducible: the systems read are the ones the loop solves
    u0 = prob.get_state().copy()

    def systems(u):
        prob.set_state(u.reshape(u0.shape))
        prob.jacobian()
        return prob.residual_vector(), prob.jacobian_csr()
    ref = kr.newton(systems, u0.ravel(), rtol=1e-6)
    assert ref.code == kr.CONVERGED and ref.its >= 2
    norms = []
    for k in range(1, ref.its + 1):                   # the device's |F| after k updates: truncated runs
        _start(prob, u0)
        with pytest.raises(RuntimeError, match="maximum"):
            prob.newton_solve(rtol=1e-30, atol=0.0, max_it=k, ksp_rtol=1e-10)
        norms.append(prob.last_report.fnorm)
        assert prob.last_report.fnorm0 == pytest.approx(ref.fnorms[0], rel=1e-12)
    print(f"[krylov] Newton |F|: reference {ref.fnorms}, device {norms}", flush=True)
    floor = 2e-6 * ref.fnorms[0]                     # (the rounding floor of F, 2e-9 |F0|, is 1e-3 of this)
    for k, fn in enumerate(norms, start=1):
        if ref.fnorms[k] > floor:
            assert fn == pytest.approx(ref.fnorms[k], rel=1e-3)
    _start(prob, u0)
    assert prob.newton_solve(rtol=1e-6, ksp_rtol=1e-10)[0] == ref.its
    assert np.abs(prob.get_state().ravel() - ref.u).max() <= 1e-6 * np.abs(ref.u).max()
    prob.close()


def test_newton_iteration_hint_right_wrong_and_unchanged_by_a_failure():
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from test_gpu_parity import _rel_rows
    prob, J, F = make_problem("init48")
    u0 = prob.get_state().copy()
    _start(prob, u0)
    n2 = prob.newton_solve(rtol=1e-3)[0]                 # first solve: no hint, every check assembles F + J
    s = prob.solver_path_stats()
    assert s["residual_only_right"] == 0 and s["residual_only_wrong"] == 0
    _start(prob, u0)
    assert prob.newton_solve(rtol=1e-3)[0] == n2
    s = prob.solver_path_stats()
    assert s["residual_only_right"] == 1 and s["residual_only_wrong"] == 0
    # a failure (max_it) leaves the hint as it was
    _start(prob, u0)
    with pytest.raises(RuntimeError, match="maximum"):
        prob.newton_solve(rtol=1e-30, atol=0.0, max_it=1)
    _start(prob, u0)
    assert prob.newton_solve(rtol=1e-3)[0] == n2
    assert prob.solver_path_stats()["residual_only_right"] == 1
    # a solve that needs one iteration more: the residual-only check was wrong, a Jacobian is assembled after all
    _start(prob, u0)
    n3 = prob.newton_solve(rtol=1e-6)[0]
    s = prob.solver_path_stats()
    print(f"[krylov] hint: {n2} iterations at 1e-3, {n3} at 1e-6, {s}", flush=True)
    assert n3 == n2 + 1 and s["residual_only_wrong"] == 1 and s["residual_only_right"] == 0
    # ... and the final check assembled F + J at the final state: the Jacobian held now is the fresh one
    U = prob.get_state()
    om = ost.build(OMesh(prob.coords, prob.cells))
    _, J_cpu = om.residual_jacobian(U, u0, u0, 5e-12, 1e30)
    assert _rel_rows(prob.jacobian_csr(), J_cpu) < 1e-10
    prob.close()


def test_watched_component_error_norm_from_the_cache():
    from oracle.controller import field_error
    prob, J, F = make_problem("init48")
    u0 = prob.get_state().copy()
    for comp in range(3):
        prob.watch_component = comp
        _start(prob, u0)
        prob.newton_solve(rtol=1e-6)                   # (sets the hint; the first solve has no residual-only check)
        _start(prob, u0)
        prob.newton_solve(rtol=1e-6)
        assert prob.solver_path_stats()["residual_only_right"] == 1
        cached = prob.field_error(comp)
        assert prob.solver_path_stats()["err_cache_served"] == 1
        U = prob.get_state()
        ref = field_error(U[:, comp], u0[:, comp])
        prob.set_state(U)                              # same bits, but the cache is dropped: the kernel of its own
        plain = prob.field_error(comp)
        assert prob.solver_path_stats()["err_cache_served"] == 1
        print(f"[krylov] watch {comp}: cached {cached!r} kernel {plain!r} float64 {ref!r}", flush=True)
        assert cached == pytest.approx(ref, rel=1e-12) and cached == pytest.approx(plain, rel=1e-12)
        # a failed solve leaves no cached value behind
        _start(prob, u0)
        with pytest.raises(RuntimeError, match="maximum"):
            prob.newton_solve(rtol=1e-30, atol=0.0, max_it=1)
        prob.field_error(comp)
        assert prob.solver_path_stats()["err_cache_served"] == 0
    prob.watch_component = None
    prob.close()


# ---- once-per-process switches: child processes ---------------------------------------------------------------------
def _child(env, what="switches", timeout=300):
    e = dict(os.environ, **env)
    out = subprocess.run([sys.executable, os.fspath(Path(__file__).resolve()), what], env=e, cwd=ROOT,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _switch_run():
    prob, J, F = make_problem("init48")
    rec = []
    for ksp in (dict(), dict(), dict(ksp_rtol=1e-10), dict(ksp_rtol=1e-10)):
        m = solve_and_measure(prob, J, -F, **ksp)
        check(str(ksp), m)
        rec.append(dict(its=m["its"], stats=m["stats"], ratio=m["ratio"], drift=m["drift"]))
    prob.close()
    return rec


@pytest.mark.parametrize("switch", ["FEDM_KRYLOV_PAIRS", "FEDM_KRYLOV_SKIP_LAST_UPDATE"])
def test_switches_read_once_per_process(switch):
    on, off = _child({switch: "1"}), _child({switch: "0"})
    key = "steps_pair" if switch == "FEDM_KRYLOV_PAIRS" else "steps_last"
    print(f"[krylov] {switch}: on {on}\n[krylov] {switch}: off {off}", flush=True)
    assert sum(r["stats"][key] for r in on) >= 1
    assert all(r["stats"][key] == 0 for r in off)
    assert [r["its"] for r in on[:2]] == [r["its"] for r in off[:2]]


if __name__ == "__main__":
    sys.path.insert(0, os.fspath(ROOT))
    sys.path.insert(0, os.fspath(HERE))
    if sys.argv[1:] == ["switches"]:
        print(json.dumps(_switch_run()))
    if sys.argv[1:] == ["nan"]:
        print(json.dumps(_nan_run()))
