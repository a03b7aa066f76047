"""Row-equilibrated GMRES on the bench's late window: scaling off / on x field-split order lower / upper, in ONE process
on ONE context, every cell from the same checkpoint (step `late_start` of the bench case).  Per cell: GMRES steps and
Newton iterations per time step, ms per step, and the state's deviation after the window from a run of the same window
at ksp_rtol 1e-10 (tools/fs_order_accuracy.py's measure: max |u - u_ref| / max |u_ref| per field).  Reported, not
judged.  Writes one JSON under profiles/.
python tools/krylov_scaling_ab.py [n=576] [late_start=200] [window=20] [out=profiles/krylov_scaling_ab.json]"""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, '.')
import numpy as np
from fedm_amd.cases import streamer

n = int(sys.argv[1]) if len(sys.argv) > 1 else 576
late = int(sys.argv[2]) if len(sys.argv) > 2 else 200
window = int(sys.argv[3]) if len(sys.argv) > 3 else 20
out = Path(sys.argv[4] if len(sys.argv) > 4 else "profiles/krylov_scaling_ab.json")

msh = streamer.mesh(n, 4.0)
prob = streamer.device_problem(msh.coords, msh.cells)
st = streamer.Stepper(prob)
st.initialise()
while st.steps < late:
    st.step()
snap = st.snapshot()
print(f"late window from step {st.steps} (t = {st.t:.3e} s), {prob.n} unknowns", flush=True)


def run(scaling, order, rtol, warm=2):
    """`window` steps from the checkpoint; the first `warm` of them (graph capture of this variant) untimed."""
    st.restore(snap)
    st.solver.parameters["krylov_residual_scaling"] = scaling
    st.solver.parameters["krylov_relative_tolerance"] = rtol
    prob.set_fieldsplit_order(order)
    rec = dict(scaling=scaling, order=order, ksp_rtol=rtol)
    try:
        for _ in range(warm):
            st.step()
        n0, l0, s0 = st.newton_iterations, st.linear_iterations, st.steps
        t0 = time.perf_counter()
        while st.steps < snap["steps"] + window:
            st.step()
        dt = time.perf_counter() - t0
        k = st.steps - s0
        rec.update(steps=k, newton_per_step=(st.newton_iterations - n0) / k, gmres_per_step=(st.linear_iterations - l0) / k,
                   ms_per_step=1e3 * dt / k, t_end=st.t)
        return rec, prob.get_state()
    except Exception as e:      # noqa: BLE001 - a cell that fails is reported as such
        rec["error"] = repr(e)
        return rec, None


ref_rec, ref = run("rows", "lower", 1e-10)
print(json.dumps(ref_rec), flush=True)
cells = []
for scaling in ("none", "rows"):
    for order in ("lower", "upper"):
        rec, U = run(scaling, order, 1e-5)
        if U is not None and ref is not None:
            rec["deviation_ions_electrons_potential"] = (np.abs(U - ref).max(axis=0) / np.abs(ref).max(axis=0)).tolist()
        cells.append(rec)
        print(json.dumps(rec), flush=True)
prob.close()
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(json.dumps(dict(mesh=n, unknowns=int(prob.n), late_start=late, window=window,
                               reference=ref_rec, cells=cells), indent=1))
print(f"written {out}")
