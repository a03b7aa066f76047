"""What the LMEA balance costs per step on the bench's glow-discharge mesh (recorded, not gated; not bench.py).

The 141 x 141 crossed mesh of bench.py's glow-discharge leg (200 225 DOFs), one ``cases.glow_discharge.Case`` with the
device pipeline stepped ``--warmup`` times, then timed in windows of ``--steps`` steps that follow one another along the
run (a Case has no checkpoint of its field table to restart from) and ALTERNATE between three routes (``--repeats``
rounds, the first one discarded as warm-up of clocks and graphs):

  none     no balance
  device   ``Case.balance()`` after every step: fedm_gd_balance, the state stays on the device
  host     ``get_state()`` + ``get_state_old()`` + ``get_gd_fields()`` (fedm_gd_get_fields) and the numpy restatement of
           tests/balance_reference.py with plain ``np.sum`` in place of ``math.fsum``, after every step

Recorded per route: ms per step of every counted window, median, min and max; per call: wall microseconds of one call
alone (its synchronisation included) on the last state; the algorithmic bytes of a call (three states 3 * 8 n_eq nv,
the field table 8 n_fields nv, cells 12 nc, coordinates 16 nv, psi 8 nv, groups nv).

    python tools/balance_ab.py
    python tools/balance_ab.py --baseline-only        # route "none" alone, with nothing this tool's other routes need:
                                                      # the same file times a commit that has no balance
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/balance_ab.py --calls-only 200
        # the call's kernels by name: gd_balance_cell_kernel, _facet_kernel, _vertex_kernel, _finish_kernel

Writes profiles/balance.json stamped with ``git describe --always --dirty`` (``--commit`` where the tree that runs has no
history).  The library is not built here: build it first.
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
    """The download route: states and field table come down, numpy forms every integral."""

    def __init__(self, case):
        sys.path.insert(0, str(ROOT / "tests"))
        import balance_reference as bref
        from fedm_amd import quadrature
        bref._sum = lambda terms, abs_terms=None: bref.Sum(float(sum(np.sum(t) for t in terms)), 0.0, 0.0)
        self.bref, self.case, self.prob = bref, case, case.prob
        self.md = self.prob.model.to_c()
        deg = self.prob.model.quadrature_degree
        self.qp, self.fqp = quadrature.triangle(deg), quadrature.interval(deg)
        self.psi = case.mesh.coords[:, 1] / case.gap
        z = case.mesh.coords[:, 1]
        self.group = np.where(np.abs(z) < 3e-16, 1, np.where(np.abs(z - case.gap) < 3e-16, 2, 0))

    def __call__(self):
        p = self.prob
        U, Uo, f = p.get_state(), p.get_state_old(), p.get_gd_fields()
        # (u_old1 has no download; u_old stands in: the same arithmetic, and this route is timed, not compared)
        ref = self.bref.reference(self.md, p.coords, p.cells, p.facet_tags(), f, U, Uo, Uo, self.case.dt.time_step,
                                  self.case.dt_old.time_step, self.qp, self.fqp, psi=self.psi, group=self.group, n_groups=2)
        return ref["content"][1].value


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
    ap.add_argument("--baseline-only", action="store_true", help="route 'none' alone, using nothing of the balance")
    ap.add_argument("--calls-only", type=int, default=0, metavar="N",
                    help="no windows: N balance calls on the warmed-up state (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the stamp, where git cannot be asked")
    a = ap.parse_args()
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=a.n, ny=a.n, T_final=1.0)
    prob = case.prob
    for _ in range(a.warmup):
        case.step()
    if a.calls_only:
        case.balance()                  # the set-up (psi, groups, the tags' lists) is made here
        t0 = time.perf_counter()
        for _ in range(a.calls_only):
            case.balance()
        print(json.dumps(dict(calls=a.calls_only, us_per_call=1e6 * (time.perf_counter() - t0) / a.calls_only)))
        return
    routes = {"none": None}
    if not a.baseline_only:
        case.balance()
        host = HostRoute(case)
        routes.update(device=case.balance, host=host)
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
    nbytes = dict(states=3 * 8 * neq * nv, field_table=8 * nf * nv, cells=12 * nc, coordinates=16 * nv, psi=8 * nv, groups=nv)
    nbytes["total"] = sum(nbytes.values())
    out = dict(commit=a.commit or commit(), mesh=f"{a.n} x {a.n} crossed", dofs=int(prob.n), vertices=nv, cells=nc,
               steps_per_window=a.steps, warmup_steps=a.warmup, baseline_only=a.baseline_only, t_end=case.t,
               algorithmic_bytes=nbytes, call=calls, routes={})
    for name, ms in windows.items():
        out["routes"][name] = dict(window_ms_per_step=ms, ms_per_step_median=statistics.median(ms),
                                   ms_per_step_min=min(ms), ms_per_step_max=max(ms))
    base = out["routes"]["none"]["ms_per_step_median"]
    for name in out["routes"]:
        if name != "none":
            out["routes"][name]["ms_per_step_over_none"] = out["routes"][name]["ms_per_step_median"] - base
    path = Path(a.out) if a.out else ROOT / "profiles" / "balance.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(dofs=out["dofs"], routes={k: {q: v[q] for q in v if q != "window_ms_per_step"}
                                                    for k, v in out["routes"].items()},
                          call=calls, bytes=nbytes["total"], written=str(path))))


if __name__ == "__main__":
    main()
