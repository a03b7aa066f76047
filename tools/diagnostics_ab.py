"""What the discharge diagnostics cost per step on the bench's mesh (recorded, not gated; not bench.py).

The refined 1 M-DOF mesh of bench.py, one device problem initialised and stepped ``--warmup`` times to bench.py's
checkpoint, then timed in windows of ``--steps`` steps that restart from that checkpoint and ALTERNATE between three
routes (``--repeats`` rounds, the first one discarded as warm-up of clocks and graphs):

  none     no diagnostics
  device   ``Stepper.diagnose()`` after every step: fedm_diagnostics, the state stays on the device
  host     what tools/refined_run.py did before: ``get_state()``, the P1 gradients in numpy, argmax near the axis,
           after every step

Recorded per route: ms per step of every counted window, median, min and max; per call: wall microseconds of
``diagnose()`` alone (its synchronisation included) on the checkpoint's state; the algorithmic bytes of a call
(state 8 n_eq nv, cells 12 nc, coordinates 16 nv, psi 8 nv, groups nv).

    python tools/diagnostics_ab.py                              # the 1 M-DOF refined mesh
    python tools/diagnostics_ab.py --spacing 2e-5 --repeats 3   # a quick look
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/diagnostics_ab.py --calls-only 200
        # the call's kernels by name: diag_cell_kernel, diag_vertex_kernel, diag_finish_kernel

Writes profiles/diagnostics.json stamped with ``git describe --always --dirty`` (``--commit`` where the tree that runs
has no history).
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
    """tools/refined_run.py's field_stats as it was: the whole state comes down, numpy does the rest."""

    def __init__(self, prob, msh, h_fine):
        self.prob = prob
        x, self.c = msh.coords, msh.cells
        a, b, d = x[self.c[:, 0]], x[self.c[:, 1]], x[self.c[:, 2]]
        det = (b[:, 0] - a[:, 0]) * (d[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (d[:, 0] - a[:, 0])
        self.G = np.stack([np.stack([b[:, 1] - d[:, 1], d[:, 0] - b[:, 0]], 1),
                           np.stack([d[:, 1] - a[:, 1], a[:, 0] - d[:, 0]], 1),
                           np.stack([a[:, 1] - b[:, 1], b[:, 0] - a[:, 0]], 1)], 1) / det[:, None, None]
        self.zc = x[self.c].mean(axis=1)[:, 1]
        self.near_axis = x[self.c].mean(axis=1)[:, 0] < 2.0 * h_fine

    def __call__(self):
        U = self.prob.get_state()
        E = -np.einsum("ca,cad->cd", U[self.c, 2], self.G)
        Em = np.linalg.norm(E, axis=1)
        k = np.argmax(np.where(self.near_axis, Em, 0.0))
        return dict(E_max_axis=float(Em[k]), z_head=float(self.zc[k]), ne_max=float(np.exp(U[:, 1].max())),
                    ni_max=float(np.exp(U[:, 0].max())))


def window(stp, snap, steps, after_step):
    import torch
    stp.restore(snap)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        stp.step()
        if after_step is not None:
            after_step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--spacing", type=float, default=4e-6, help="finest spacing of the refined mesh [m] (bench.py: 4e-6)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=6, help="rounds over the routes; the first is not counted")
    ap.add_argument("--calls-only", type=int, default=0, metavar="N",
                    help="no windows: N diagnostics calls on the checkpoint's state (for a kernel trace)")
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
    prob = streamer.device_problem(msh.coords, msh.cells)
    stp = streamer.Stepper(prob)
    stp.initialise()
    for _ in range(a.warmup):
        stp.step()
    snap = stp.snapshot()
    row = stp.diagnose()                # the set-up (psi, groups) is made here, outside every window
    if a.calls_only:
        t0 = time.perf_counter()
        for _ in range(a.calls_only):
            stp.diagnose()
        print(json.dumps(dict(calls=a.calls_only, us_per_call=1e6 * (time.perf_counter() - t0) / a.calls_only)))
        return
    host = HostRoute(prob, msh, a.spacing)
    routes = {"none": None, "device": stp.diagnose, "host": host}
    windows = {name: [] for name in routes}
    for r in range(a.repeats):
        for name, after in routes.items():         # alternating: none, device, host, none, ...
            ms = window(stp, snap, a.steps, after)
            if r > 0:
                windows[name].append(ms)
    stp.restore(snap)
    calls = {}
    for name, fn in (("device", stp.diagnose), ("host", host)):
        us = []
        for _ in range(30):
            t0 = time.perf_counter()
            fn()
            us.append(1e6 * (time.perf_counter() - t0))
        calls[name] = dict(us_median=statistics.median(us), us_min=min(us), us_max=max(us))
    nv, nc, neq = int(msh.coords.shape[0]), int(msh.cells.shape[0]), prob.n_eq
    nbytes = dict(state=8 * neq * nv, cells=12 * nc, coordinates=16 * nv, psi=8 * nv, groups=nv)
    nbytes["total"] = sum(nbytes.values())
    out = dict(commit=a.commit or commit(), mesh="refined", spacing=a.spacing, dofs=int(prob.n), vertices=nv, cells=nc,
               steps_per_window=a.steps, warmup_steps=a.warmup, mesh_seconds=t_mesh, algorithmic_bytes=nbytes,
               row_at_checkpoint=row, host_row_at_checkpoint=host(), call=calls, routes={})
    for name, ms in windows.items():
        out["routes"][name] = dict(window_ms_per_step=ms, ms_per_step_median=statistics.median(ms),
                                   ms_per_step_min=min(ms), ms_per_step_max=max(ms))
    base = out["routes"]["none"]["ms_per_step_median"]
    for name in ("device", "host"):
        out["routes"][name]["ms_per_step_over_none"] = out["routes"][name]["ms_per_step_median"] - base
    path = Path(a.out) if a.out else ROOT / "profiles" / "diagnostics.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(dofs=out["dofs"], routes={k: {q: v[q] for q in v if q != "window_ms_per_step"}
                                                    for k, v in out["routes"].items()},
                          call=calls, bytes=nbytes["total"], written=str(path))))


if __name__ == "__main__":
    main()
