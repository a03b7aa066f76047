"""The refined Krylov step (the second Gram-Schmidt pass queued behind the step it refines, krylov.cpp) and the hint
slots per Newton iteration, on the 48x48 problems of test_gpu_krylov.py and with that file's conditions: every linear
solve is held to ``true <= 2 tol`` at ``ksp_rtol = 1e-5`` and to ``its == steps_used == launched - dropped`` (`check`).

The linear solves of tests 1-3 are run once (`runs`) and shared:

* context P (assembly by global colouring: J is reproducible bit for bit; degree-10 species polynomial), right-hand
  side ``b = J s`` with s = 1 on every species entry and 0 on the potential: solves A (fresh context, no hint), B, C;
  then ``J x = -F`` twice (S1 with the refinement predicted in vain, S2 after the bit was cleared);
* context Q, fresh, same settings, P's state, its hierarchy rebuilt like P's (`_reproducible`): ``J x = -F`` twice (T0 without a hint, T1 with its own count as the hint).

Which system: the refined graphs reach the first four steps of a solve's first cycle.  With the right-hand side 1 on one
Dirichlet row (test_second_pass's) no cancellation falls there: measured on an MI355X for the rows 0, 3, 24, 48, 49 and
97 of ``streamer.dirichlet`` at restart 30 (49-119 steps in 2-5 cycles, 30-44 second passes, none within reach, no solve
within one cycle) and for row 3 at restarts 8, 4, 3, 2 (no convergence within 10 000 steps) -- neither the row nor the
restart brings it within reach.  A cancellation in step 0 needs ``J M^-1 v_0 = v_0`` to 1e-4, as in the first Newton
system of an early time step on the bench's mesh: on init48 the smooth species right-hand side above with the degree-10
polynomial does it (measured: 2 steps, 1 second pass, at step 0; degree 6 and 8: none, degree 12: 2), and ``-F`` needs
none with that polynomial either.

What a hint changes is how steps are grouped into launches, never a kernel or its operands, so x of S1 (hint: the
``b = J s`` solve's count), of S2 and of T1 (hint: their own count) must agree bit for bit when the early-exit kernels
touch nothing.
"""
import numpy as np
import pytest

from test_gpu_krylov import DRIFT_BOUND, G_BOUND, _start, check, make_problem, solve_and_measure  # noqa: F401

pytestmark = pytest.mark.gpu

LAUNCHES = ("steps_single", "steps_pair", "steps_last", "steps_dropped", "updates_made_up", "steps_ahead",
            "steps_used", "second_passes", "second_passes_device", "cycles", "verified")


def _floor(J, m, b):
    """test_second_pass's floor: the float64 evaluation of the residual itself carries (w + 2) eps | |J| |x| + |b| | on
    the device and on the host alike (w entries a row)."""
    width = int(np.diff(J.indptr).max())
    return 2.0 * (width + 2) * np.finfo(float).eps * float(np.linalg.norm(abs(J) @ np.abs(m["x"]) + np.abs(b)))


def _reproducible(prob, U):
    """Everything a solve reads, formed from the state U under the assembly by global colouring: make_problem builds
    the multigrid hierarchy from a potential block assembled by LDS patches, whose sums differ in their last bits from
    context to context, and so do the cycles of two contexts."""
    from fedm_amd.device import chebyshev_weights
    prob.set_state(U, U, U)
    prob.set_assembly("colour")
    prob.clear_multigrid()
    prob.setup_multigrid(nu=1, omega=0.85, max_coarse=40)       # (test_gpu_krylov._streamer48's)
    prob.set_fieldsplit(chebyshev_weights(10))
    prob.jacobian()
    return prob.jacobian_csr(), prob.residual_vector()


@pytest.fixture(scope="module")
def runs():
    out = {}
    prob, _, _ = make_problem("init48")
    U = prob.get_state().copy()
    J, F = _reproducible(prob, U)
    s = np.zeros((prob.nv, prob.n_eq))
    s[:, :-1] = 1.0
    b = J @ s.ravel()
    for name in "ABC":
        out[name] = solve_and_measure(prob, J, b)
    for name in ("S1", "S2"):
        out[name] = solve_and_measure(prob, J, -F)
    prob.close()
    fresh, _, _ = make_problem("init48")
    Jq, Fq = _reproducible(fresh, U)     # (P's state: the initial Poisson solve is not reproducible to the last bit either)
    out["same_system"] = bool(np.array_equal(Jq.data, J.data) and np.array_equal(Jq.indices, J.indices)
                              and np.array_equal(Fq, F))
    for name in ("T0", "T1"):
        out[name] = solve_and_measure(fresh, Jq, -Fq)
    fresh.close()
    out.update(J=J, F=F, b=b)
    return out


def test_device_pass_equals_host_pass(runs):
    J, b = runs["J"], runs["b"]
    A, B, C = runs["A"], runs["B"], runs["C"]
    for label, m in (("A: no hint, host pass", A), ("B: predicted, device pass", B), ("C: once more", C)):
        check("b = J s, " + label, m, residual_floor=_floor(J, m, b))
        assert m["stats"]["breakdowns"] == 0
    a, s = A["stats"], B["stats"]
    assert a["second_passes"] >= 1 and a["second_passes_device"] == 0
    assert s["second_passes_device"] >= 1
    assert s["second_passes"] == s["second_passes_device"]
    assert s["steps_dropped"] == 0
    assert B["its"] == A["its"]
    assert np.linalg.norm(J @ (B["x"] - A["x"])) <= 2.0 * A["tol"] * (1.0 + G_BOUND["right"])
    assert {k: C["stats"][k] for k in LAUNCHES} == {k: s[k] for k in LAUNCHES}
    assert C["its"] == B["its"]


def test_wrong_prediction_costs_only_launches(runs):
    assert runs["same_system"]                # the colour assembly gave both contexts the same J and F, bit for bit
    S1, S2, T0, T1 = runs["S1"], runs["S2"], runs["T0"], runs["T1"]
    for label, m in (("S1: refinement predicted in vain", S1), ("S2: bit cleared", S2), ("T0: fresh, no hint", T0),
                     ("T1: fresh, own hint", T1)):
        check("J x = -F, " + label, m)
        assert m["stats"]["second_passes"] == 0 and m["stats"]["second_passes_device"] == 0
    assert S1["its"] == T1["its"] == S2["its"] == T0["its"]
    assert np.array_equal(S1["x"], T1["x"])          # the early-exit kernels touched nothing
    assert np.array_equal(S2["x"], T1["x"])
    # the bit was cleared: with the same hint the further solve launches what the context that never refined launches
    assert {k: S2["stats"][k] for k in LAUNCHES} == {k: T1["stats"][k] for k in LAUNCHES}


def test_host_path_still_there(runs):
    """The refined path's own guard cannot be made to fail from outside; the path it falls back to is the one solve A
    took (no prediction yet): test_second_pass's assertions, beside B for the comparison."""
    A, B = runs["A"], runs["B"]
    check("b = J s, host pass", A, residual_floor=_floor(runs["J"], A, runs["b"]))
    assert A["stats"]["second_passes"] >= 1 and A["stats"]["breakdowns"] == 0 and A["stats"]["second_passes_device"] == 0
    assert A["stats"]["second_passes"] == B["stats"]["second_passes"]


def test_hints_per_newton_iteration():
    prob, _, F = make_problem("init48")
    u0 = prob.get_state().copy()

    def newton():
        _start(prob, u0)
        its = prob.newton_solve(rtol=1e-6)[0]
        s = prob.solver_path_stats()
        print(f"[refine] newton: {its} iterations, {prob.last_report.linear_iterations} Krylov steps, "
              f"{ {k: v for k, v in s.items() if v} }", flush=True)
        return its, prob.last_report.linear_iterations, s, prob.get_state().copy()
    n1, l1, _, u1 = newton()
    n2, l2, s2, u2 = newton()
    assert (n2, l2) == (n1, l1)
    assert s2["steps_dropped"] == 0 and s2["updates_made_up"] == 0 and s2["steps_ahead"] >= 1
    assert np.abs(u2 - u1).max() <= 1e-6 * np.abs(u1).max()
    # a solve outside the Newton loop, to another tolerance: it has a slot of its own
    prob.set_state(u0, u0, u0)
    prob.jacobian()
    code = prob.linear_solve(-prob.residual_vector(), ksp_rtol=1e-10)[3]
    assert code == 0
    n3, l3, s3, _ = newton()
    assert (n3, l3) == (n2, l2)
    assert {k: s3[k] for k in LAUNCHES} == {k: s2[k] for k in LAUNCHES}
    prob.close()


def test_snapshot_restores_every_slot():
    from fedm_amd.cases import streamer
    msh = streamer.mesh(48, 4.0)
    run = streamer.Stepper(streamer.device_problem(msh.coords, msh.cells))
    run.initialise()

    def two_steps():
        before = run.prob.solver_path_stats()
        for _ in range(2):
            run.step()
        after = run.prob.solver_path_stats()
        return {k: after[k] - before[k] for k in after}
    for _ in range(3):
        run.step()
    snap = run.snapshot()
    first = two_steps()
    for _ in range(3):
        run.step()
    run.restore(snap)
    again = two_steps()
    run.prob.close()
    print(f"[refine] two steps from the snapshot: { {k: v for k, v in first.items() if v} }", flush=True)
    assert again == first
    assert first["steps_dropped"] == 0 and again["steps_dropped"] == 0
