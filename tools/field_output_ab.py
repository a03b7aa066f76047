"""What field output costs per step on the bench's mesh (recorded, not gated; not bench.py).

The refined 1 M-DOF mesh of bench.py, one device problem initialised and stepped ``--warmup`` times to bench.py's
checkpoint, then timed in windows of ``--steps`` steps that restart from that checkpoint and ALTERNATE between three
routes (``--repeats`` rounds, the first one discarded as warm-up of clocks and graphs):

  none     no output
  device   after every step ``E_norm`` and ``charge`` as nodal fields and an axis profile (``E_z``, ``n_e`` at
           ``--points`` points of r = 0) from the device: two fedm_fields calls, the state stays there
  host     the same quantities the way the scripts formed them: ``get_state()``, the P1 gradient cell by cell and its
           lumped projection in numpy, the densities' charge, the profile by interpolation

Recorded per route: ms per step of every counted window, median, min and max; per call: wall microseconds of the
route's output alone (its synchronisation included) on the checkpoint's state, and for the host route how much of it is
``get_state()``; the bytes a device call brings back.

    python tools/field_output_ab.py                              # the 1 M-DOF refined mesh
    python tools/field_output_ab.py --spacing 2e-5 --repeats 3   # a quick look
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/field_output_ab.py --calls-only 200
        # the calls' kernels by name: fields_cell_kernel, fields_vertex_kernel, fields_probe_kernel

Writes profiles/field_output.json stamped with ``git describe --always --dirty`` (``--commit`` where the tree that runs
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


class DeviceRoute:
    def __init__(self, stp, points):
        self.stp = stp
        self.nodal = ("E_norm", "charge")
        self.profile = ("E_z", "density:electrons")
        self.points = points
        self.stp.prob.fields_setup()
        self.stp.prob.probe_setup(points)

        self.seconds_library = []

    def __call__(self):
        prob = self.stp.prob
        fields = prob.fields(self.nodal)
        lib = prob.last_fields_call_seconds
        profile = prob.fields(self.profile, nodal=False, probes=True, species_names=("ions", "electrons"))
        self.seconds_library.append(lib + prob.last_fields_call_seconds)
        return fields.nodal, profile.probes


class HostRoute:
    """The whole state comes down, numpy does the rest: cell gradients, their lumped projection, the charge, the
    profile."""

    def __init__(self, prob, msh, points):
        from fedm_amd import field_output
        from fedm_amd.physical_constants import elementary_charge
        self.prob, self.e = prob, elementary_charge
        x, self.c = msh.coords, msh.cells
        a, b, d = x[self.c[:, 0]], x[self.c[:, 1]], x[self.c[:, 2]]
        det = (b[:, 0] - a[:, 0]) * (d[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (d[:, 0] - a[:, 0])
        self.G = np.stack([np.stack([b[:, 1] - d[:, 1], d[:, 0] - b[:, 0]], 1),
                           np.stack([d[:, 1] - a[:, 1], a[:, 0] - d[:, 0]], 1),
                           np.stack([a[:, 1] - b[:, 1], b[:, 0] - a[:, 0]], 1)], 1) / det[:, None, None]
        self.area6 = np.abs(det) / 6.0
        self.nv = x.shape[0]
        self.flat = self.c.ravel()
        self.m = np.bincount(self.flat, weights=np.repeat(self.area6, 3), minlength=self.nv)
        cell, self.w = field_output.locate_points(x, self.c, points)
        self.at = self.c[cell]
        self.seconds_get_state = []

    def project(self, f):
        return np.bincount(self.flat, weights=np.repeat(f * self.area6, 3), minlength=self.nv) / self.m

    def __call__(self):
        t0 = time.perf_counter()
        U = self.prob.get_state()
        self.seconds_get_state.append(time.perf_counter() - t0)
        E = -np.einsum("ca,cad->cd", U[self.c, 2], self.G)
        e_norm = self.project(np.linalg.norm(E, axis=1))
        n_e = np.exp(U[:, 1])
        charge = self.e * (np.exp(U[:, 0]) - n_e)
        e_z = self.project(E[:, 1])
        profile = np.stack([(self.w * e_z[self.at]).sum(axis=1), (self.w * n_e[self.at]).sum(axis=1)])
        return np.stack([e_norm, charge]), profile


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
    ap.add_argument("--points", type=int, default=512, help="points of the axis profile")
    ap.add_argument("--calls-only", type=int, default=0, metavar="N",
                    help="no windows: N device outputs on the checkpoint's state (for a kernel trace)")
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
    z = np.linspace(0.0, streamer.BOX, a.points)
    points = np.column_stack([np.zeros_like(z), z])
    t0 = time.perf_counter()
    device = DeviceRoute(stp, points)       # the set-up (lists, lumped mass, point location) is made here, outside every window
    t_setup = time.perf_counter() - t0
    if a.calls_only:
        t0 = time.perf_counter()
        for _ in range(a.calls_only):
            device()
        print(json.dumps(dict(calls=a.calls_only, us_per_output=1e6 * (time.perf_counter() - t0) / a.calls_only)))
        return
    host = HostRoute(prob, msh, points)
    routes = {"none": None, "device": device, "host": host}
    windows = {name: [] for name in routes}
    for r in range(a.repeats):
        for name, after in routes.items():         # alternating: none, device, host, none, ...
            ms = window(stp, snap, a.steps, after)
            if r > 0:
                windows[name].append(ms)
    stp.restore(snap)
    calls, results = {}, {}
    host.seconds_get_state.clear()
    device.seconds_library.clear()
    for name, fn in (("device", device), ("host", host)):
        us = []
        for _ in range(30):
            t0 = time.perf_counter()
            results[name] = fn()
            us.append(1e6 * (time.perf_counter() - t0))
        calls[name] = dict(us_median=statistics.median(us), us_min=min(us), us_max=max(us))
    calls["host"]["us_get_state_median"] = 1e6 * statistics.median(host.seconds_get_state)
    calls["device"]["us_library_median"] = 1e6 * statistics.median(device.seconds_library)
    # the two routes form the same quantities (E_norm and E_z: lumped projections of the cell field)
    agree = {}
    for k, name in enumerate(("E_norm", "charge")):
        d, h = results["device"][0][k], results["host"][0][k]
        agree[name] = float(np.abs(d - h).max() / np.abs(h).max())
    for k, name in enumerate(("E_z profile", "n_e profile")):
        d, h = results["device"][1][k], results["host"][1][k]
        agree[name] = float(np.abs(d - h).max() / np.abs(h).max())
    nv, nc, neq = int(msh.coords.shape[0]), int(msh.cells.shape[0]), prob.n_eq
    nbytes = dict(device_read_back=8 * (2 * nv + 2 * a.points), host_read_back=8 * neq * nv)
    out = dict(commit=a.commit or commit(), mesh="refined", spacing=a.spacing, dofs=int(prob.n), vertices=nv, cells=nc,
               steps_per_window=a.steps, warmup_steps=a.warmup, mesh_seconds=t_mesh, setup_seconds=t_setup,
               profile_points=a.points, read_back_bytes=nbytes, routes_agree_relative=agree, call=calls, routes={})
    for name, ms in windows.items():
        out["routes"][name] = dict(window_ms_per_step=ms, ms_per_step_median=statistics.median(ms),
                                   ms_per_step_min=min(ms), ms_per_step_max=max(ms))
    base = out["routes"]["none"]["ms_per_step_median"]
    for name in ("device", "host"):
        out["routes"][name]["ms_per_step_over_none"] = out["routes"][name]["ms_per_step_median"] - base
    path = Path(a.out) if a.out else ROOT / "profiles" / "field_output.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(dofs=out["dofs"], routes={k: {q: v[q] for q in v if q != "window_ms_per_step"}
                                                    for k, v in out["routes"].items()},
                          call=calls, agree=agree, written=str(path))))


if __name__ == "__main__":
    main()
