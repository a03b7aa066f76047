"""What a dielectric layer costs per step on the bench's streamer mesh (recorded, not gated; not bench.py).

The refined 1 M-DOF mesh of bench.py, the deck's model with the electrons' 'flux source' wall on both electrodes (the
constants of tests/wall_flux_reference.py), once as it is and once with the cathode coated (``--thickness``,
``--eps-r``): two device problems in one process, each initialised, stepped ``--warmup`` times and checkpointed; every
window restarts from its problem's checkpoint (tools/circuit_ab.py).  Windows of ``--steps`` steps ALTERNATE between the
two (``--repeats`` rounds, the first one discarded as warm-up of clocks and graphs).  Recorded per route: ms per step of
every counted window, median, min and max, and the Krylov steps and Newton iterations per step -- the mirrored part of
the layer's Jacobian is outside the field split's multigrid block, so the count is what to watch; the accept call
alone (wall microseconds, synchronised) and dielectric_charge() with its read-back.

    python tools/dielectric_ab.py

Writes profiles/dielectric.json stamped with ``git describe --always --dirty`` (``--commit`` where the tree that runs
has no history).  The library is not built here: build it first.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from circuit_ab import commit, timed  # noqa: E402


def wall_problem(msh, dielectric):
    """cases/streamer.device_problem with the electrons' 'flux source' wall on the electrodes (the ions of the deck are
    immobile: they meet no wall)."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Walls
    from fedm_amd.mesh import Marking_boundaries, Mesh
    m = Mesh(msh.coords, msh.cells)
    dofs, vals = streamer.dirichlet(m.coords)
    if dielectric is not None:          # the coated cathode's values leave: the conductor is behind the layer, at 0 V
        keep = np.abs(m.coords[dofs // 3, 1]) > 3e-16
        dofs, vals = dofs[keep], vals[keep]
    lfa = streamer.model()
    lfa.bc_kind = [["zero flux", "flux source"], ["zero flux", "flux source"], ["zero flux"] * 2, ["zero flux"] * 2]
    lfa.walls = Walls(vth=[[0.0, 1e5]] * 2 + [[0.0, 0.0]] * 2, ref=[[1.0, 0.3], [1.0, 0.0], [1.0, 1.0], [1.0, 1.0]],
                      gamma=[0.0] * 4, emits=[False, True], is_ion=[False, False])
    lfa.dielectric = dielectric
    return DeviceProblem(m.coords, m.cells, lfa, facet_tags=Marking_boundaries(m, streamer.BOUNDARIES),
                         dirichlet_dofs=dofs, dirichlet_vals=vals)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--spacing", type=float, default=4e-6, help="finest spacing of the refined mesh [m] (bench.py: 4e-6)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1, help="steps before the checkpoint")
    ap.add_argument("--repeats", type=int, default=6, help="rounds over the two routes; the first is not counted")
    ap.add_argument("--thickness", type=float, default=1e-4, help="the layer's thickness [m]")
    ap.add_argument("--eps-r", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the stamp, where git cannot be asked")
    a = ap.parse_args()
    import torch
    from fedm_amd.cases import streamer
    from fedm_amd.device import Dielectric
    channel = (0.0, 100.0 * 4e-6) + streamer.CHANNEL[2:]
    msh = streamer.refined_mesh(a.spacing, growth=0.1, channel=channel)
    routes = {}
    for name, layer in (("wall", None), ("wall+layer", Dielectric(thickness={1: a.thickness}, eps_r={1: a.eps_r}))):
        prob = wall_problem(msh, layer)
        stp = streamer.Stepper(prob)
        stp.initialise()
        for _ in range(a.warmup):
            stp.step()
        routes[name] = dict(prob=prob, stp=stp, snap=stp.snapshot(), ms=[], krylov=[], newton=[])

    def window(r, steps, count):
        stp = r["stp"]
        stp.restore(r["snap"])          # (the layer's charge and its predecessor come back with it)
        k0, n0 = stp.linear_iterations, stp.newton_iterations
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            stp.step()
        torch.cuda.synchronize()
        if count:
            r["ms"].append(1e3 * (time.perf_counter() - t0) / steps)
            r["krylov"].append((stp.linear_iterations - k0) / steps)
            r["newton"].append((stp.newton_iterations - n0) / steps)

    for rnd in range(a.repeats):
        for r in routes.values():           # alternating: wall, wall+layer, wall, ...
            window(r, a.steps, rnd > 0)
    lay = routes["wall+layer"]["prob"]

    def accept():
        lay.dielectric_accept()
        torch.cuda.synchronize()
    calls = dict(accept=timed(accept, 30), charge_read_back=timed(lambda: lay.dielectric_charge(vertices=False), 30))
    calls["state"] = {k: {str(t): v for t, v in d.items()} for k, d in lay.dielectric_charge(vertices=False).items()
                      if isinstance(d, dict)}
    entry = dict(commit=a.commit or commit(), mesh=f"refined, spacing {a.spacing}", dofs=int(lay.n), vertices=int(lay.nv),
                 cells=int(lay.nc), steps_per_window=a.steps, thickness_m=a.thickness, eps_r=a.eps_r, call=calls, routes={},
                 launched={k: r["prob"].launched_assembly()["jacobian"] for k, r in routes.items()})
    for name, r in routes.items():
        entry["routes"][name] = dict(window_ms_per_step=r["ms"], ms_per_step_median=statistics.median(r["ms"]),
                                     ms_per_step_min=min(r["ms"]), ms_per_step_max=max(r["ms"]),
                                     krylov_steps_per_step=statistics.median(r["krylov"]),
                                     newton_iterations_per_step=statistics.median(r["newton"]))
    base = entry["routes"]["wall"]
    entry["routes"]["wall+layer"]["ms_per_step_over_wall"] = entry["routes"]["wall+layer"]["ms_per_step_median"] - base["ms_per_step_median"]
    entry["routes"]["wall+layer"]["krylov_ratio"] = entry["routes"]["wall+layer"]["krylov_steps_per_step"] / base["krylov_steps_per_step"]
    path = Path(a.out) if a.out else ROOT / "profiles" / "dielectric.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    whole = json.loads(path.read_text()) if path.exists() else {}
    whole["streamer"] = entry
    path.write_text(json.dumps(whole, indent=1) + "\n")
    print(json.dumps(dict(dofs=entry["dofs"], call={k: v for k, v in calls.items() if k != "state"},
                          routes={k: {q: v[q] for q in v if q != "window_ms_per_step"} for k, v in entry["routes"].items()},
                          written=str(path))))


if __name__ == "__main__":
    main()
