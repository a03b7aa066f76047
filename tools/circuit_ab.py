"""What the external circuit costs per step on the bench's meshes (recorded, not gated; not bench.py).

``--case streamer``: the refined 1 M-DOF mesh of bench.py, one device problem initialised, stepped ``--warmup`` times and
checkpointed; every window restarts from the checkpoint (tools/currents_ab.py).  ``--case glow``: the 141 x 141 crossed
mesh of bench.py's glow-discharge leg, one ``cases.glow_discharge.Case`` whose windows follow one another along the run.
Windows of ``--steps`` steps ALTERNATE between three routes (``--repeats`` rounds, the first one discarded as warm-up of
clocks and graphs):

  none     no circuit: the ideal source, the step of the parent commit
  device   ``fedm.External_circuit``: measure after every accepted step, advance and apply before every solve attempt;
           nothing is read back
  host     the same loop closed on the host: ``currents()`` (fedm_currents and its read-back) after every step, the numpy
           advance of tests/circuit_reference.py with the conductance left at 0 (the host has none without a further pass)
           and ``set_dirichlet_values`` before every solve attempt

The ballast is small enough (``--ballast``, default 1 kOhm) for the host's lagged update to stay bounded: the routes are
timed, not compared.  Recorded per route: ms per step of every counted window, median, min and max; wall microseconds
of one measure + advance pair alone and of one advance with its read-back.

    python tools/circuit_ab.py --case streamer
    python tools/circuit_ab.py --case glow
    python tools/circuit_ab.py --case glow --baseline-only --label parent_1 --commit HASH
        # route "none" alone, with nothing the other routes need: the same file, copied into a checkout of the parent
        # commit, times that commit

Writes profiles/circuit.json (one entry per case, merged into the file) stamped with ``git describe --always --dirty``
(``--commit`` where the tree that runs has no history).  The library is not built here: build it first.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def commit():
    try:
        return subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:       # noqa: BLE001 - a tarball has no history
        return "unknown"


def timed(fn, n):
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        us.append(1e6 * (time.perf_counter() - t0))
    return dict(us_median=statistics.median(us), us_min=min(us), us_max=max(us))


class HostCircuit:
    """The loop closed on the host: a read-back of the currents, a scalar update, an upload of the Dirichlet values."""

    def __init__(self, prob, sources, R, U0, entries, base_values, steps_of):
        sys.path.insert(0, str(ROOT / "tests"))
        import circuit_reference as circ
        self.circ, self.prob, self.sources, self.R, self.steps_of = circ, prob, sources, np.asarray(R, dtype=float), steps_of
        self.hist = [np.asarray(U0, dtype=float)] * 2
        self.entries, self.base_values, self.t, self.cur, self.U = entries, base_values, 0.0, prob.currents(), None

    def before_solve(self):
        dt, dt_old = self.steps_of()
        n = self.R.size
        V = [f(self.t) for f in self.sources]
        out = self.circ.advance(self.cur.raw["conduction"], np.zeros((n, n)), self.cur.raw["capacitance"], self.hist[0],
                                self.hist[1], dt, dt_old, V, self.R, np.zeros(n))
        self.U = out["U"]
        vals = self.base_values(self.t)
        vals = np.where(self.entries >= 0, self.U[np.maximum(self.entries, 0)], vals)
        self.prob.set_dirichlet_values(vals)

    def accept(self):
        self.cur = self.prob.currents()
        self.hist = [self.U, self.hist[0]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", choices=["streamer", "glow"], default="glow")
    ap.add_argument("--spacing", type=float, default=4e-6, help="streamer: finest spacing of the refined mesh [m] (bench.py: 4e-6)")
    ap.add_argument("--n", type=int, default=141, help="glow: cells per side of the crossed mesh (bench.py: 141)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=None, help="steps before the windows (streamer 1, glow 5)")
    ap.add_argument("--repeats", type=int, default=6, help="rounds over the routes; the first is not counted")
    ap.add_argument("--ballast", type=float, default=1.0e3, help="series resistance [ohm]")
    ap.add_argument("--baseline-only", action="store_true", help="route 'none' alone, using nothing of the circuit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the stamp, where git cannot be asked")
    ap.add_argument("--label", default=None, help="suffix of the entry's key, to keep several runs of one case apart")
    a = ap.parse_args()
    import torch
    lmea = a.case == "glow"
    if lmea:
        from fedm_amd.cases import glow_discharge as gdc
        case = gdc.Case(nx=a.n, ny=a.n, T_final=1.0)
        prob, step, restart, problem = case.prob, case.step, lambda: None, case.problem
        steps_of = lambda: (case.dt.time_step, case.dt_old.time_step)        # noqa: E731
        for _ in range(5 if a.warmup is None else a.warmup):
            step()
        mesh_name = f"{a.n} x {a.n} crossed"
        sources = [lambda t: case.U_w * (1.0 - np.exp(-t / 1e-9)), lambda t: 0.0]
        R, driven, base_values, holder = [a.ballast, 0.0], 0, case.dirichlet_values, case
        U0_of = lambda: [sources[0](case.t), 0.0]                             # noqa: E731
    else:
        from fedm_amd.cases import streamer
        channel = (0.0, 100.0 * 4e-6) + streamer.CHANNEL[2:]
        msh = streamer.refined_mesh(a.spacing, growth=0.1, channel=channel)
        prob = streamer.device_problem(msh.coords, msh.cells)
        stp = streamer.Stepper(prob)
        stp.initialise()
        for _ in range(1 if a.warmup is None else a.warmup):
            stp.step()
        snap = stp.snapshot()
        step, restart, problem = stp.step, lambda: stp.restore(snap), stp.problem
        steps_of = lambda: (stp.dt.time_step, stp.dt_old.time_step)          # noqa: E731
        mesh_name = f"refined, spacing {a.spacing}"
        sources = [lambda t: 0.0, lambda t: streamer.U_W]
        initial = prob._dvals.copy()
        R, driven, base_values, holder = [0.0, a.ballast], 1, (lambda t: initial), stp
        U0_of = lambda: [0.0, streamer.U_W]                                  # noqa: E731
    plain_before, plain_timed = getattr(problem, "before_solve", None), list(getattr(holder, "_timed", []))

    def window(steps, after_step):
        restart()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
            if after_step is not None:
                after_step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    def use_none():
        problem.before_solve, holder._timed = plain_before, plain_timed
        if not lmea and not a.baseline_only:
            prob.set_dirichlet_values(base_values(0.0))
        return None

    routes, calls = {"none": use_none}, {}
    if not a.baseline_only:
        from fedm_amd import functions as ff
        electrodes = ff.Electrode_currents(prob, boundary_tags=(1, 2))

        def make_device():
            circuit = ff.External_circuit(prob, electrodes, sources, R, 0.0, U0_of())
            problem.before_solve = plain_before
            circuit.bind(problem)
            holder._timed = plain_timed + [circuit]
            return circuit.accept

        def make_host():
            host = HostCircuit(prob, sources, R, U0_of(), prob.circuit_entries.astype(np.int64), base_values, steps_of)

            def before():
                if plain_before is not None:
                    plain_before()
                host.before_solve()
            problem.before_solve, holder._timed = before, plain_timed + [host]
            return host.accept
        routes.update(device=make_device, host=make_host)
    windows = {name: [] for name in routes}
    for r in range(a.repeats):
        for name, make in routes.items():         # alternating: none, device, host, none, ...
            ms = window(a.steps, make())
            if r > 0:
                windows[name].append(ms)
    use_none()
    restart()
    if not a.baseline_only:
        circuit = ff.External_circuit(prob, electrodes, sources, R, 0.0, U0_of())
        prob.set_step(*steps_of())

        def pair():
            circuit.accept()
            circuit.advance(0.0)
            torch.cuda.synchronize()
        calls["measure_and_advance"] = timed(pair, 30)
        calls["advance_with_read_back"] = timed(lambda: circuit.advance(0.0, read=True), 30)
        calls["currents_read_back"] = timed(prob.currents, 30)
        s = circuit.state()
        calls["state"] = dict(U=s.U.tolist(), conduction_A=s.conduction.tolist(), conductance_S=s.conductance.tolist(), flag=s.flag)
        use_none()
    entry = dict(commit=a.commit or commit(), mesh=mesh_name, dofs=int(prob.n), vertices=int(prob.nv), cells=int(prob.nc),
                 steps_per_window=a.steps, ballast_ohm=a.ballast, driven_electrode=driven, baseline_only=a.baseline_only,
                 call=calls, routes={})
    for name, ms in windows.items():
        entry["routes"][name] = dict(window_ms_per_step=ms, ms_per_step_median=statistics.median(ms), ms_per_step_min=min(ms),
                                     ms_per_step_max=max(ms))
    base = entry["routes"]["none"]["ms_per_step_median"]
    for name in entry["routes"]:
        if name != "none":
            entry["routes"][name]["ms_per_step_over_none"] = entry["routes"][name]["ms_per_step_median"] - base
    path = Path(a.out) if a.out else ROOT / "profiles" / "circuit.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    whole = json.loads(path.read_text()) if path.exists() else {}
    whole[a.case + ("_baseline" if a.baseline_only else "") + (f"_{a.label}" if a.label else "")] = entry
    path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(dict(case=a.case, dofs=entry["dofs"], call=calls,
                          routes={k: {q: v[q] for q in v if q != "window_ms_per_step"} for k, v in entry["routes"].items()},
                          written=str(path))))


if __name__ == "__main__":
    main()
