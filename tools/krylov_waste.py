"""Krylov steps a time step launches against those it uses, on the headline case of bench.py (refined unstructured
mesh, 4 um in the channel, 1 023 840 DOFs): per step the deltas of `solver_path_stats()` and the Newton iterations, for
the 20 steps after one warm-up step and for 20 steps from step 200 (the developed streamer).

usage: python tools/krylov_waste.py [OUT.json] [--late-start N]      (N = 0: no late window)
Prints one JSON document (and writes it to OUT.json): {"early": {"steps": [...], "sum": {...}}, "late": ...}."""
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

KEYS = ("steps_used", "steps_single", "steps_pair", "steps_last", "steps_dropped", "second_passes",
        "second_passes_device", "updates_made_up", "steps_ahead")


def window(runner, steps):
    rows = []
    for _ in range(steps):
        before = runner.prob.solver_path_stats()
        n0, l0 = runner.newton_iterations, runner.linear_iterations
        runner.step()
        after = runner.prob.solver_path_stats()
        row = {k: after[k] - before[k] for k in KEYS if k in after}
        row.update(step=runner.steps, newton=runner.newton_iterations - n0, linear=runner.linear_iterations - l0)
        rows.append(row)
    total = {k: sum(r[k] for r in rows) for k in rows[0] if k != "step"}
    return {"steps": rows, "sum": total}


def main():
    args = sys.argv[1:]
    late_start = 200
    if "--late-start" in args:
        i = args.index("--late-start")
        late_start = int(args[i + 1])
        del args[i:i + 2]
    import __graft_entry__ as entry
    entry.build()                      # before the GPU is touched (bench.py's library_ready)
    from fedm_amd.cases import streamer
    spacing = 4e-6
    channel = (0.0, 100.0 * spacing) + streamer.CHANNEL[2:]
    with tempfile.TemporaryDirectory(prefix="fedm_mesh_") as tmp:
        msh = streamer.refined_mesh(spacing, growth=0.1, xml_path=Path(tmp) / "mesh.xml", channel=channel)
    runner = streamer.Stepper(streamer.device_problem(msh.coords, msh.cells))
    runner.initialise()
    runner.step()                      # the warm-up step of `bench.py --warmup 1`
    out = {"case": f"bench.py headline: refined mesh, {runner.total_dofs} DOFs; 1 warm-up step, then 20 steps",
           "early": window(runner, 20)}
    if late_start > 0:
        while runner.steps < late_start:
            runner.step()
        out["late"] = window(runner, 20)
    text = json.dumps(out, indent=1)
    print(text)
    if args:
        Path(args[0]).parent.mkdir(parents=True, exist_ok=True)
        Path(args[0]).write_text(text + "\n")


if __name__ == "__main__":
    main()
