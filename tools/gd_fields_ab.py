"""What the LMEA field output costs per step on the bench's glow-discharge mesh (recorded, not gated; not bench.py).

The 141 x 141 crossed mesh of bench.py's glow-discharge leg (200 225 DOFs), one ``cases.glow_discharge.Case`` with the
device pipeline stepped ``--warmup`` times, then timed in windows of ``--steps`` steps that follow one another along the
run and ALTERNATE between three routes (``--repeats`` rounds, the first one discarded as warm-up of clocks and graphs),
as tools/balance_ab.py does:

  none     no output
  device   ``Case.fields()`` after every step: mean_energy, E_norm, source:electrons and joule as nodal fields plus a
           512-point axis profile of each (fedm_gd_fields; the states and the table stay on the device)
  host     ``get_state()`` + ``get_gd_fields()`` (fedm_gd_get_fields) and numpy for the same four fields and the same
           profile: the point functions of tests/balance_reference.py through tests/gd_fields_reference.py's integrands,
           added with ``np.bincount`` in place of ``math.fsum``, lumped

Recorded per route: ms per step of every counted window, median, min and max; per call: wall microseconds of one call
alone (its synchronisation and read-back included) on the last state; the algorithmic bytes of a call (one state
8 n_eq nv, the rows of the field table bal_point reads 8 (n_fields - 2 n_r + the reactions' rows asked for) nv -- all of
them here -- cells 12 nc, coordinates 16 nv, the corner entries written and read 2 * 24 nc per projected request, the
results 8 nvp per request and their read-back).

    python tools/gd_fields_ab.py
    python tools/gd_fields_ab.py --baseline-only      # route "none" alone, with nothing this tool's other routes need:
                                                      # the same file times a commit that has no LMEA field output
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gd_fields_ab.py --calls-only 200
        # the call's kernels by name: gd_fields_cell_kernel, gd_fields_vertex_kernel, fields_probe_kernel

Writes profiles/gd_fields.json stamped with ``git describe --always --dirty`` (``--commit`` where the tree that runs has
no history).  The library is not built here: build it first.
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
NAMES = ["mean_energy", "E_norm", "source:electrons", "joule"]
AXIS_POINTS = 512


def commit():
    try:
        return subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:       # noqa: BLE001 - a tarball has no history
        return "unknown"


class HostRoute:
    """The download route: the state and the field table come down, numpy forms the four fields and the profile."""

    def __init__(self, case, points):
        sys.path.insert(0, str(ROOT / "tests"))
        import gd_fields_reference as gfr
        from fedm_amd import field_output, quadrature
        self.gfr, self.case, self.prob = gfr, case, case.prob
        self.md = self.prob.model.to_c()
        self.qp = quadrature.triangle(self.prob.model.quadrature_degree)
        cell, self.w = field_output.locate_points(self.prob.coords, self.prob.cells, points)
        self.at = self.prob.cells[cell]
        x = self.prob.coords[self.prob.cells]
        d1, d2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
        self.m = np.bincount(self.prob.cells.ravel(), weights=np.repeat(np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]) / 6.0, 3),
                             minlength=self.prob.nv)

    def __call__(self):
        p, ns = self.prob, self.prob.model.n_species
        U, f = p.get_state(), p.get_gd_fields()
        r = self.gfr.Restatement.__new__(self.gfr.Restatement)        # (no per-vertex lists: bincount adds)
        r.md, r.fields, r.qp, r.fault, r.cells = self.md, f, self.qp, None, p.cells
        r.nv, r.nc, r.ns, r.nr = p.nv, p.nc, ns, p.model.n_reactions
        r.x, r.detJ, r.G = self.gfr.bref.geometry(p.coords, p.cells)
        out = [np.exp(U[:, 0] - U[:, ns - 1])]
        for kind, index in (("e_norm", 0), ("source", ns - 1), ("joule", 0)):
            integrands, _ = r.cell_integrands(U, kind, index)
            b = np.zeros(p.nv)
            for (phi, W), addends in zip(r.points(), integrands):
                fq = W * sum(addends)
                for a in range(3):
                    b += np.bincount(p.cells[:, a], weights=fq * phi[a], minlength=p.nv)
            out.append(b / self.m)
        X = np.stack(out)
        return X, (self.w[None] * X[:, self.at]).sum(axis=2)


def window(case, steps, after_step):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        case.step()
        if after_step is not None:
            after_step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=141, help="cells per side of the crossed mesh (bench.py: 141)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=6, help="rounds over the routes; the first is not counted")
    ap.add_argument("--baseline-only", action="store_true", help="route 'none' alone, using nothing of the field output")
    ap.add_argument("--calls-only", type=int, default=0, metavar="N",
                    help="no windows: N field-output calls on the warmed-up state (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the stamp, where git cannot be asked")
    a = ap.parse_args()
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=a.n, ny=a.n, T_final=1.0)
    prob = case.prob
    for _ in range(a.warmup):
        case.step()
    z = np.linspace(0.0, case.gap, AXIS_POINTS)
    points = np.column_stack([0.0 * z, z])
    device = lambda: case.fields(NAMES, probes=points)      # noqa: E731
    if a.calls_only:
        device()                        # the set-up (vertex lists, lumped mass, the points) is made here
        t0 = time.perf_counter()
        for _ in range(a.calls_only):
            device()
        print(json.dumps(dict(calls=a.calls_only, us_per_call=1e6 * (time.perf_counter() - t0) / a.calls_only)))
        return
    routes = {"none": None}
    if not a.baseline_only:
        first = device()
        host = HostRoute(case, points)
        X, P = host()
        worst = max(float(np.abs(first[n] - X[k]).max() / np.abs(X[k]).max()) for k, n in enumerate(NAMES))
        routes.update(device=device, host=host)
    windows = {name: [] for name in routes}
    for r in range(a.repeats):
        for name, after in routes.items():         # alternating: none, device, host, none, ...
            ms = window(case, a.steps, after)
            if r > 0:
                windows[name].append(ms)
    calls = {}
    for name, fn in routes.items():
        if fn is None:
            continue
        us = []
        for _ in range(30 if name == "device" else 5):
            t0 = time.perf_counter()
            fn()
            us.append(1e6 * (time.perf_counter() - t0))
        calls[name] = dict(us_median=statistics.median(us), us_min=min(us), us_max=max(us))
    nv, nc, neq, nf = prob.nv, prob.nc, prob.n_eq, prob.model.n_fields
    projected = 3
    nbytes = dict(state=8 * neq * nv, field_table=8 * nf * nv, cells=12 * nc, coordinates=16 * nv,
                  corner_entries=2 * 24 * nc * projected, vertex_lists=4 * (nv + 1) + 12 * nc, results=8 * nv * len(NAMES),
                  read_back=8 * nv * len(NAMES) + 8 * AXIS_POINTS * len(NAMES))
    nbytes["total"] = sum(nbytes.values())
    out = dict(commit=a.commit or commit(), mesh=f"{a.n} x {a.n} crossed", dofs=int(prob.n), vertices=nv, cells=nc,
               steps_per_window=a.steps, warmup_steps=a.warmup, baseline_only=a.baseline_only, t_end=case.t,
               fields=NAMES, axis_points=AXIS_POINTS, algorithmic_bytes=nbytes, call=calls, routes={})
    if not a.baseline_only:
        out["device_against_host_worst_relative_difference"] = worst
    for name, ms in windows.items():
        out["routes"][name] = dict(window_ms_per_step=ms, ms_per_step_median=statistics.median(ms),
                                   ms_per_step_min=min(ms), ms_per_step_max=max(ms))
    base = out["routes"]["none"]["ms_per_step_median"]
    for name in out["routes"]:
        if name != "none":
            out["routes"][name]["ms_per_step_over_none"] = out["routes"][name]["ms_per_step_median"] - base
    path = Path(a.out) if a.out else ROOT / "profiles" / "gd_fields.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(dofs=out["dofs"], routes={k: {q: v[q] for q in v if q != "window_ms_per_step"}
                                                    for k, v in out["routes"].items()},
                          call=calls, bytes=nbytes["total"], written=str(path))))


if __name__ == "__main__":
    main()
