"""Time steps with and without photoionisation on the bench's mesh (recorded, not gated; not bench.py).

The refined 1 M-DOF mesh of bench.py, three device problems on it -- the benchmark's model, the same with the
photoionisation source of ``cases/streamer.default_photoionization`` preconditioned by its hierarchies, and with Jacobi
alone -- each initialised and stepped ``--warmup`` times to bench.py's checkpoint, then timed in windows of ``--steps``
steps that restart from that checkpoint and ALTERNATE between the problems (``--repeats`` rounds, the first one
discarded as warm-up of clocks and graphs).  Recorded per problem: ms per step of every window, Newton and Krylov counts;
per photoionisation problem: wall microseconds per update (everything ``DeviceProblem.photo_update`` does, its
synchronisation included), of an update that finds its start converged (load vector, one residual and one norm per
term, table write: everything but CG iterations), CG iterations per term and update, V-cycles; per problem the F + J
assembly kernel it takes and ``fedm_time_kernel`` kind 0 of it.

    python tools/photo_ab.py                              # the 1 M-DOF refined mesh
    python tools/photo_ab.py --spacing 2e-5 --repeats 3   # a quick look
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/photo_ab.py --updates-only 40
        # the update's kernels by name (photo_cell_load_kernel, photo_vertex_sum_kernel: the load vector; ell_spmv_kernel,
        # scalar_cg_dots_kernel, scalar_cg_update_kernel, ...: the solves; photo_table_kernel: the table write)

Writes profiles/photoionization.json stamped with ``git describe --always --dirty`` (``--commit`` where the tree that
runs has no history).
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def commit():
    try:
        return subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:       # noqa: BLE001 - a tarball has no history
        return "unknown"


class Timed:
    """A stepper whose photoionisation updates are timed and counted (wall clock around DeviceProblem.photo_update)."""

    def __init__(self, name, stp):
        self.name, self.stp, self.prob = name, stp, stp.prob
        self.update_us, self.update_its = [], []
        if self.prob._has_photo():
            inner = self.prob.photo_update

            def timed_update():
                t0 = time.perf_counter()
                its = inner()
                self.update_us.append(1e6 * (time.perf_counter() - t0))
                self.update_its.append(list(its))
                return its
            self.prob.photo_update = timed_update

    def window(self, snap, steps):
        import torch
        self.stp.restore(snap)
        self.update_us, self.update_its = [], []
        n0, l0 = self.stp.newton_iterations, self.stp.linear_iterations
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.stp.step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        rec = dict(ms_per_step=1e3 * el / steps, newton=self.stp.newton_iterations - n0,
                   krylov=self.stp.linear_iterations - l0, t_end=self.stp.t)
        if self.update_us:
            rec.update(updates=len(self.update_us), update_us=list(self.update_us), cg_iterations=list(self.update_its))
        return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--spacing", type=float, default=4e-6, help="finest spacing of the refined mesh [m] (bench.py: 4e-6)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=6, help="rounds over the problems; the first is not counted")
    ap.add_argument("--updates-only", type=int, default=0, metavar="N",
                    help="no windows: N steps of the photoionisation problem alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the stamp, where git cannot be asked")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    from fedm_amd.cases import streamer
    t0 = time.perf_counter()
    channel = (0.0, 100.0 * 4e-6) + streamer.CHANNEL[2:]
    msh = streamer.refined_mesh(a.spacing, growth=0.1, channel=channel)
    t_mesh = time.perf_counter() - t0
    variants = {"plain": None, "photo": streamer.default_photoionization(),
                "photo_jacobi": streamer.default_photoionization(multigrid=False, max_it=50000)}
    if a.updates_only:
        variants = {"photo": variants["photo"]}
    runs, setup_s = {}, {}
    for name, ph in variants.items():
        t0 = time.perf_counter()
        prob = streamer.device_problem(msh.coords, msh.cells, photoionization=ph)
        stp = streamer.Stepper(prob)
        stp.initialise()
        for _ in range(a.warmup):
            stp.step()
        runs[name] = (Timed(name, stp), stp.snapshot())
        setup_s[name] = time.perf_counter() - t0
    if a.updates_only:
        run, snap = runs["photo"]
        rec = run.window(snap, a.updates_only)
        print(json.dumps(dict(steps=a.updates_only, ms_per_step=rec["ms_per_step"],
                              update_us_median=statistics.median(rec["update_us"]))))
        return
    out = dict(commit=a.commit or commit(), mesh="refined", spacing=a.spacing, dofs=int(runs["plain"][0].prob.n),
               vertices=int(msh.coords.shape[0]), steps_per_window=a.steps, warmup_steps=a.warmup,
               mesh_seconds=t_mesh, setup_seconds=setup_s, problems={})
    windows = {name: [] for name in runs}
    for r in range(a.repeats):
        for name, (run, snap) in runs.items():          # alternating: plain, photo, photo_jacobi, plain, ...
            if name == "photo_jacobi" and r > 1:        # (thousands of CG steps an update: one counted window of it)
                continue
            rec = run.window(snap, a.steps)
            if r > 0:
                windows[name].append(rec)
    for name, (run, snap) in runs.items():
        prob = run.prob
        ms = [w["ms_per_step"] for w in windows[name]]
        rec = dict(window_ms_per_step=ms, ms_per_step_median=statistics.median(ms), ms_per_step_min=min(ms),
                   ms_per_step_max=max(ms), newton_per_window=windows[name][-1]["newton"],
                   krylov_per_window=windows[name][-1]["krylov"], assembly_variant=prob.sizes()["assembly_variant"],
                   patch_threads=prob.sizes()["patch_threads"])
        run.stp.restore(snap)
        rec["assembly_FJ_ms"] = prob.time_kernel(0, 50)
        rec["assembly_F_ms"] = prob.time_kernel(2, 50)
        if prob._has_photo():
            us = [u for w in windows[name] for u in w["update_us"]]
            its = [i for w in windows[name] for i in w["cg_iterations"]]
            n_terms = len(prob.model.photoionization.c)
            rec.update(update_us_median=statistics.median(us), update_us_min=min(us), update_us_max=max(us),
                       updates_per_window=windows[name][-1]["updates"],
                       cg_iterations_per_update=[sum(i[m] for i in its) / len(its) for m in range(n_terms)],
                       cg_iterations_last_window=windows[name][-1]["cg_iterations"],
                       hierarchy_levels=prob.photo_levels, stats=prob.photo_stats())
            # an update that finds its start converged: load vector, a residual and a norm per term, table write
            run.stp.restore(snap)
            prob.photo_update()
            idle = []
            for _ in range(20):
                prob._photo_stale = True
                t0 = time.perf_counter()
                prob.photo_update()
                idle.append(1e6 * (time.perf_counter() - t0))
            rec["update_without_cg_iterations_us_median"] = statistics.median(idle)
            rec["cg_iterations_us_median"] = rec["update_us_median"] - rec["update_without_cg_iterations_us_median"]
        out["problems"][name] = rec
    plain = out["problems"]["plain"]["ms_per_step_median"]
    for name in ("photo", "photo_jacobi"):
        out["problems"][name]["ms_per_step_over_plain"] = out["problems"][name]["ms_per_step_median"] / plain
    path = Path(a.out) if a.out else ROOT / "profiles" / "photoionization.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    brief = {k: {q: v[q] for q in v if q in ("ms_per_step_median", "ms_per_step_min", "ms_per_step_max", "assembly_variant",
                                              "assembly_FJ_ms", "update_us_median", "update_without_cg_iterations_us_median",
                                              "cg_iterations_per_update", "ms_per_step_over_plain")}
             for k, v in out["problems"].items()}
    print(json.dumps(dict(dofs=out["dofs"], mesh_seconds=t_mesh, setup_seconds=setup_s, problems=brief, written=str(path))))


if __name__ == "__main__":
    main()
