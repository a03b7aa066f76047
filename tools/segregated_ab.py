"""Coupled against segregated time steps over the same simulated time span (recorded, not gated; not bench.py).

Both runs start from ONE device checkpoint (``Stepper.snapshot`` after ``--start`` coupled steps: 200 = the developed
streamer of bench.py's ``late_window``), run with the step controller on until ``--span`` seconds later, and are
compared: steps/s, accepted and rejected attempts, the dt sequence, Newton / Krylov / CG counts per step,
``eps0 / (e mu_e n_e) / dt`` of the END state for the largest and the smallest step of the run (the stability margin of
the explicit coupling: the dielectric relaxation time over the step; the densest plasma of a growing streamer is the last
one, and reading the state every step would sit in the timing) and the per-component difference of the two end states.  The kernel times of ``fedm_time_kernel`` kinds 0, 2, 6, 7
come with it.

    python tools/segregated_ab.py --mesh refined            # the 1 M-DOF refined mesh of bench.py
    python tools/segregated_ab.py --mesh tensor --cells 576
    python tools/segregated_ab.py --mesh tensor --cells 96 --start 20 --span 5e-11     # a quick look

Writes profiles/segregated_ab_<mesh>.json stamped with ``git describe --always --dirty`` (``--commit`` where the tree
that runs has no history).
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

EPS0, QE = 8.8541878128e-12, 1.602176634e-19


def commit():
    try:
        return subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:       # noqa: BLE001 - a tarball has no history
        return "unknown"


def relaxation_margin(U, dt, mu_e):
    """eps0 / (e mu_e n_e) / dt at the largest electron density of the state."""
    return EPS0 / (QE * mu_e * float(np.exp(U[:, 1].max()))) / dt


def mobility():
    """mu_e of the deck at the applied field U_W / BOX (the head's field is a few times larger and mu_e falls with E:
    the cautious side for the margin)."""
    from fedm_amd.cases import streamer
    from fedm_amd.termsum import parse
    return float(parse(streamer.MU_E)(streamer.U_W / streamer.BOX))


def run_span(stp, snap, coupling, t_end, mu_e):
    stp.restore(snap)
    stp.solver.parameters["coupling"] = coupling
    prob = stp.prob
    prob.segregated_stats(reset=True)
    open(stp.error_file, "w").close()
    rec = dict(dt=[], newton=[], krylov=[], cg=[])
    n0, l0 = stp.newton_iterations, stp.linear_iterations
    t0 = time.perf_counter()
    while stp.t < t_end * (1.0 - 1e-9):
        cg_before = prob.segregated_stats()["cg_iterations"]
        n_before, l_before = stp.newton_iterations, stp.linear_iterations
        stp.step()
        rec["dt"].append(stp.dt_old.time_step)
        rec["newton"].append(stp.newton_iterations - n_before)
        rec["krylov"].append(stp.linear_iterations - l_before)
        rec["cg"].append(prob.segregated_stats()["cg_iterations"] - cg_before)
    wall = time.perf_counter() - t0
    U = prob.get_state().reshape(prob.nv, -1)
    attempts = len(stp.log_rows())
    steps = len(rec["dt"])
    margins = [relaxation_margin(U, d, mu_e) for d in (max(rec["dt"]), min(rec["dt"]))]
    return U, dict(coupling=coupling, steps=steps, attempts=attempts, rejected=attempts - steps, wall_s=wall,
                   steps_per_s=steps / wall, t_end=stp.t, newton_per_step=(stp.newton_iterations - n0) / steps,
                   krylov_per_step=(stp.linear_iterations - l0) / steps, cg_per_step=sum(rec["cg"]) / steps,
                   relaxation_time_over_dt_at_end=min(margins), dt_sequence=rec["dt"], newton=rec["newton"],
                   krylov=rec["krylov"], cg=rec["cg"], segregated_stats=prob.segregated_stats())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", choices=["refined", "tensor"], default="refined")
    ap.add_argument("--cells", type=int, default=576, help="tensor mesh: cells per side")
    ap.add_argument("--spacing", type=float, default=4e-6, help="refined mesh: finest spacing [m]")
    ap.add_argument("--start", type=int, default=200, help="coupled steps before the checkpoint")
    ap.add_argument("--span", type=float, default=2.5e-10, help="simulated seconds both runs cover")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the stamp, where git cannot be asked")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    from fedm_amd.cases import streamer
    if a.mesh == "refined":
        channel = (0.0, 100.0 * a.spacing) + streamer.CHANNEL[2:]
        msh = streamer.refined_mesh(a.spacing, growth=0.1, channel=channel)
        name = "refined"
    else:
        msh = streamer.mesh(a.cells, 4.0)
        name = f"tensor{a.cells}"
    prob = streamer.device_problem(msh.coords, msh.cells)
    stp = streamer.Stepper(prob)
    stp.initialise()
    for _ in range(a.start):
        stp.step()
    snap = stp.snapshot()
    t_end = stp.t + a.span
    mu_e = mobility()
    kernels = {f"kind{k}_ms": prob.time_kernel(k, 50) for k in (0, 2, 6, 7)}
    stp.restore(snap)
    out = dict(commit=a.commit or commit(), mesh=name, dofs=int(prob.n), start_steps=a.start, t_start=snap["t"], span=a.span,
               kernel_ms=kernels, runs={})
    states = {}
    for coupling in ("coupled", "uncoupled", "coupled", "uncoupled"):      # twice: the first pass warms both paths up
        U, rec = run_span(stp, snap, coupling, t_end, mu_e)
        states[coupling] = U
        out["runs"][coupling] = rec
    diff = np.abs(states["uncoupled"] - states["coupled"]).max(axis=0) / np.abs(states["coupled"]).max(axis=0)
    out["end_state_difference"] = [float(v) for v in diff]
    path = Path(a.out) if a.out else ROOT / "profiles" / f"segregated_ab_{name}.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    brief = {k: {q: v[q] for q in ("steps", "rejected", "steps_per_s", "newton_per_step", "krylov_per_step",
                                   "cg_per_step", "relaxation_time_over_dt_at_end")} for k, v in out["runs"].items()}
    print(json.dumps(dict(mesh=name, dofs=out["dofs"], kernel_ms=kernels, runs=brief,
                          end_state_difference=out["end_state_difference"], written=str(path))))


if __name__ == "__main__":
    main()
