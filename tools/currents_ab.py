"""What the electrode currents cost per step on the bench's meshes (recorded, not gated; not bench.py).

``--case streamer``: the refined 1 M-DOF mesh of bench.py, one device problem initialised, stepped ``--warmup`` times and
checkpointed; every window restarts from the checkpoint (tools/diagnostics_ab.py).  ``--case glow``: the 141 x 141 crossed
mesh of bench.py's glow-discharge leg, one ``cases.glow_discharge.Case`` whose windows follow one another along the run
(tools/balance_ab.py).  Windows of ``--steps`` steps ALTERNATE between three routes (``--repeats`` rounds, the first one
discarded as warm-up of clocks and graphs):

  none     no currents
  device   ``currents()`` with the two electrodes' solved potentials after every step: fedm_currents, the state stays
           on the device
  host     ``get_state()`` / ``get_state_old()`` (and ``get_gd_fields()``) and the numpy restatement of
           tests/currents_reference.py with plain ``np.sum`` in place of ``math.fsum``, after every step, with the same
           two potentials (windows of ``--host-steps`` steps: a call takes a multiple of a step).  An approximation of
           that route from below: no entry point downloads u_old1, so u_old is downloaded twice in its place (the same
           traffic and arithmetic; the numbers are timed, not compared), and the sums are numpy's

Recorded per route: ms per step of every counted window, median, min and max; per call: wall microseconds of one call
alone (its synchronisation included) for 1, 2, 4 and 8 given potentials and for the two solved ones; the one-off set-up:
seconds of the host's assembly and hierarchy, of the device's solve, its CG iterations per potential and level sizes.

    python tools/currents_ab.py --case streamer
    python tools/currents_ab.py --case glow
    python tools/currents_ab.py --case glow --baseline-only --label parent_1 --commit HASH
        # route "none" alone, with nothing the other routes need: the same file, copied into a checkout of a commit that
        # has no currents, times that commit; --label names the entry (<case>_baseline_<label>), so alternating runs of
        # two trees keep an entry each
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/currents_ab.py --case glow --calls-only 200

Writes profiles/currents.json (one entry per case, merged into the file) stamped with ``git describe --always --dirty``
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


class HostRoute:
    """The download route: the states (and the field table) come down, numpy forms every integral."""

    def __init__(self, prob, psi, lmea, steps_of):
        sys.path.insert(0, str(ROOT / "tests"))
        import currents_reference as cref
        cref._sum = lambda arrays: cref.Sum(float(sum(np.sum(a) for a in arrays)), 0.0)
        self.cref, self.prob, self.psi, self.lmea, self.steps_of = cref, prob, psi, lmea, steps_of
        if lmea:
            from fedm_amd import quadrature
            self.md = prob.model.to_c()
            self.qp = quadrature.triangle(prob.model.quadrature_degree)
        else:
            from oracle import streamer as ost
            from oracle.mesh import Mesh as OMesh
            self.om = ost.build(OMesh(prob.coords, prob.cells))

    def __call__(self):
        p = self.prob
        U, Uo = p.get_state(), p.get_state_old()
        Uo1 = p.get_state_old()     # (u_old1 has no download; u_old stands in: the same traffic and arithmetic, timed, not compared)
        dt, dt_old = self.steps_of()
        if self.lmea:
            ref = self.cref.lmea_reference(self.md, p.coords, p.cells, p.get_gd_fields(), U, Uo, Uo1, dt, dt_old, self.qp, self.psi)
        else:
            ref = self.cref.lfa_reference(self.om, U, Uo, Uo1, dt, dt_old, self.psi)
        return ref["conduction"][0].value


def timed(fn, n):
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        us.append(1e6 * (time.perf_counter() - t0))
    return dict(us_median=statistics.median(us), us_min=min(us), us_max=max(us))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", choices=["streamer", "glow"], default="glow")
    ap.add_argument("--spacing", type=float, default=4e-6, help="streamer: finest spacing of the refined mesh [m] (bench.py: 4e-6)")
    ap.add_argument("--n", type=int, default=141, help="glow: cells per side of the crossed mesh (bench.py: 141)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=None, help="steps before the windows (streamer 1, glow 5)")
    ap.add_argument("--repeats", type=int, default=6, help="rounds over the routes; the first is not counted")
    ap.add_argument("--baseline-only", action="store_true", help="route 'none' alone, using nothing of the currents")
    ap.add_argument("--calls-only", type=int, default=0, metavar="N", help="no windows: N calls on the warmed-up state (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the stamp, where git cannot be asked")
    ap.add_argument("--label", default=None, help="suffix of the entry's key, to keep several runs of one case apart")
    a = ap.parse_args()
    import torch
    lmea = a.case == "glow"
    if lmea:
        from fedm_amd.cases import glow_discharge as gdc
        case = gdc.Case(nx=a.n, ny=a.n, T_final=1.0)
        prob, step, restart = case.prob, case.step, lambda: None
        steps_of = lambda: (case.dt.time_step, case.dt_old.time_step)        # noqa: E731
        for _ in range(5 if a.warmup is None else a.warmup):
            step()
        mesh_name = f"{a.n} x {a.n} crossed"
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
        step, restart = stp.step, lambda: stp.restore(snap)
        steps_of = lambda: (stp.dt.time_step, stp.dt_old.time_step)          # noqa: E731
        mesh_name = f"refined, spacing {a.spacing}"

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

    routes, setup, calls = {"none": (None, a.steps)}, {}, {}
    if not a.baseline_only:
        t0 = time.perf_counter()
        its = prob.currents_setup(boundary_tags=(1, 2))
        t_all = time.perf_counter() - t0
        levels, rhs, _ = prob.currents_system
        t0 = time.perf_counter()
        prob.currents_solve(levels, rhs)              # from the solved potentials: the upload and a check of the residual alone
        t_again = time.perf_counter() - t0
        psi = prob.currents_psi()
        prob.currents_setup(boundary_tags=(1, 2))
        setup = dict(seconds_host_assembly_hierarchy_upload_and_solve=t_all, seconds_upload_and_converged_solve=t_again,
                     cg_iterations=its, levels=prob.currents_levels,
                     max_abs_psi0_plus_psi1_minus_1=float(np.abs(psi[0] + psi[1] - 1.0).max()))
        if a.calls_only:
            t0 = time.perf_counter()
            for _ in range(a.calls_only):
                prob.currents()
            print(json.dumps(dict(calls=a.calls_only, us_per_call=1e6 * (time.perf_counter() - t0) / a.calls_only)))
            return
        host = HostRoute(prob, psi, lmea, steps_of)
        routes.update(device=(prob.currents, a.steps), host=(host, a.host_steps))
    windows = {name: [] for name in routes}
    for r in range(a.repeats):
        for name, (after, steps) in routes.items():         # alternating: none, device, host, none, ...
            ms = window(steps, after)
            if r > 0:
                windows[name].append(ms)
    restart()
    if not a.baseline_only:
        calls["solved_2"] = timed(prob.currents, 30)
        calls["host_2"] = timed(host, 3)
        z = prob.coords[:, 1] / prob.coords[:, 1].max()
        r = prob.coords[:, 0] / prob.coords[:, 0].max()
        for n in (1, 2, 4, 8):
            prob.currents_setup(potentials=np.stack([(1.0 + 0.3 * k) * z + 0.1 * k * r * r for k in range(n)]))
            calls[f"given_{n}"] = timed(prob.currents, 30)
        prob.currents_setup(potentials=psi)
        calls["us_per_extra_potential"] = (calls["given_8"]["us_median"] - calls["given_1"]["us_median"]) / 7.0
    entry = dict(commit=a.commit or commit(), mesh=mesh_name, dofs=int(prob.n), vertices=int(prob.nv), cells=int(prob.nc),
                 steps_per_window=a.steps, host_steps_per_window=a.host_steps, baseline_only=a.baseline_only, setup=setup,
                 call=calls, routes={})
    for name, ms in windows.items():
        entry["routes"][name] = dict(window_ms_per_step=ms, ms_per_step_median=statistics.median(ms), ms_per_step_min=min(ms),
                                     ms_per_step_max=max(ms))
    base = entry["routes"]["none"]["ms_per_step_median"]
    for name in entry["routes"]:
        if name != "none":
            entry["routes"][name]["ms_per_step_over_none"] = entry["routes"][name]["ms_per_step_median"] - base
    path = Path(a.out) if a.out else ROOT / "profiles" / "currents.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    whole = json.loads(path.read_text()) if path.exists() else {}
    whole[a.case + ("_baseline" if a.baseline_only else "") + (f"_{a.label}" if a.label else "")] = entry
    path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(dict(case=a.case, dofs=entry["dofs"], setup=setup, call=calls,
                          routes={k: {q: v[q] for q in v if q != "window_ms_per_step"} for k, v in entry["routes"].items()},
                          written=str(path))))


if __name__ == "__main__":
    main()
