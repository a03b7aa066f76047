"""The fused facet-and-Dirichlet launch against the two launches it replaces, on one GPU.

On one GPU with the LDS-patch assembly and no row shared between a facet and a Dirichlet dof, launch_assemble leaves
the facets to launch_finalize, which runs them and the Dirichlet / padding rows as ONE kernel
(boundary_dirichlet_kernel, boundary.hip).  FEDM_FUSED_BOUNDARY=0 keeps the two-launch form: boundary_kernel<.., ATOMIC>
behind the volume kernel, then dirichlet_kernel.  The switch is read once per process, so the two-launch figures come
from ONE fresh child process (this file run as a script, under a time limit of its own) and the fused ones from the
test process.  Both forms share the accumulation sinks, the unit-row writer and the model-flag dispatch; this holds
them to each other.

Mesh: oracle.mesh.rectangle_right with n = 9 -- 100 vertices in two 64-row slices, 28 padding vertices behind them,
facets and Dirichlet dofs in both slices.  State: the initial state with smoke()'s perturbation, dt = 5e-12.
Models: the closed-form streamer and the tabulated deck (a TAB instance through the shared dispatch).

Compared: F of residual(), J after two Jacobian assemblies in a row (a kept plane shows on the second), and the F the
F + J assembly leaves.  Tolerances: those of tests/test_gpu_rank_assembly.py for the same quantities -- both forms sum
the same terms with atomics in a run-dependent order -- F 1e-11 of max |F|, J 1e-10 of each row's largest entry.
The Dirichlet rows are stores, not sums: exactly equal, F = u - value and a unit row in both forms.  The padding rows
lie behind the n_vertices rows the C ABI returns and a one-GPU context has no identity vertices, so neither can be
read here; the padding vertices share slice 1 with the vertices 64..99, whose rows are compared.

The launch record (fedm_launched_assembly) names the volume kernel only; it is asserted to be an LDS-patch one in both
processes, which with one GPU, tagged facets and Dirichlet values on the potential alone is what the fused launch takes.

Measured on an MI355X (both cases together 5 s, the child process included): streamer (one-pass) F 3.1e-17, J 3.8e-16;
tabulated (lds-patches) F 3.1e-17, J 2.4e-16.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
N = 9
DT = (5e-12, 1e30)
DECKS = {"streamer": None, "tabulated": "tabulated_model"}


def _mesh_and_states():
    from oracle import streamer as ost
    from oracle.mesh import rectangle_right
    mesh = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, N, N)
    U0 = ost.initial_state(ost.build(mesh))
    x, y = mesh.coords[:, 0] / ost.BOX, mesh.coords[:, 1] / ost.BOX
    U1 = U0.copy()
    U1[:, 0] += 0.05 * np.sin(7.0 * x) * np.cos(5.0 * y)
    U1[:, 1] += 0.05 * np.cos(3.0 * x) * np.sin(4.0 * y)
    return mesh, U1, U0


def _assemble(mesh, U1, U0, deck):
    """F, J (dense), the F of the F + J assembly and the launched volume variants of one context."""
    from fedm_amd.cases import streamer
    prob = streamer.device_problem(mesh.coords, mesh.cells, deck_model=deck)
    try:
        prob.set_state(U1, U0, U0)
        prob.set_step(*DT)
        F, _ = prob.residual()
        prob.jacobian()
        prob.jacobian()
        J = prob.jacobian_csr().toarray()
        F_fj = prob.residual_vector()
        launched = prob.launched_assembly()
        variants = [str(launched[k]["variant"]) for k in ("residual", "jacobian")]
        # the slices (64 device-ordered vertices each) that hold Dirichlet vertices and vertices of the Neumann walls
        slice_of = prob._inv >> 6
        dirichlet_slices = np.unique(slice_of[streamer.dirichlet(mesh.coords)[0] // 3])
        r = mesh.coords[:, 0]
        facet_slices = np.unique(slice_of[(r == 0.0) | (r == streamer.BOX)])
        return dict(F=F, J=J, F_fj=F_fj, variants=np.array(variants), padding=prob.sizes()["n_slices"] * 64 - prob.nv,
                    dirichlet_slices=dirichlet_slices, facet_slices=facet_slices)
    finally:
        prob.close()


@pytest.fixture(scope="module")
def inputs():
    assert os.environ.get("FEDM_FUSED_BOUNDARY", "1")[:1] != "0", "the test process must run the fused launch"
    return _mesh_and_states()


@pytest.fixture(scope="module")
def two_launches(inputs, tmp_path_factory):
    """Every case in the two-launch form, from one child process."""
    out = tmp_path_factory.mktemp("boundary_rows") / "two_launches.npz"
    env = dict(os.environ, FEDM_FUSED_BOUNDARY="0", PYTHONPATH=os.pathsep.join([str(ROOT), str(HERE)]))
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(out)], env=env, cwd=str(ROOT),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return np.load(out)


@pytest.mark.parametrize("case", list(DECKS))
def test_fused_launch_equals_the_two_launches(inputs, two_launches, case):
    from fedm_amd.cases import streamer
    mesh, U1, U0 = inputs
    fused = _assemble(mesh, U1, U0, DECKS[case])
    two = {k: two_launches[f"{case}_{k}"] for k in ("F", "J", "F_fj", "variants", "padding")}
    dofs, vals = streamer.dirichlet(mesh.coords)
    Fscale = np.abs(two["F"]).max()
    eF = np.abs(fused["F"] - two["F"]).max() / Fscale
    eFJ = np.abs(fused["F_fj"] - two["F_fj"]).max() / Fscale
    rows = np.maximum(np.abs(two["J"]).max(axis=1), 1e-300)
    eJ = (np.abs(fused["J"] - two["J"]) / rows[:, None]).max()
    print(f"[boundary rows] {case}: F {eF:.2e} F of F+J {eFJ:.2e} J {eJ:.2e}; launched {[str(v) for v in fused['variants']]} "
          f"(fused) / {[str(v) for v in two['variants']]} (two launches); {dofs.size} Dirichlet dofs, {int(fused['padding'])} "
          f"padding vertices, {mesh.coords.shape[0]} vertices", flush=True)
    assert mesh.coords.shape[0] == 100 and int(fused["padding"]) == 28 and int(two["padding"]) == 28
    assert all(v.startswith("lds-patches") for v in fused["variants"]), fused["variants"]
    assert list(fused["variants"]) == list(two["variants"])
    assert dofs.size == 2 * (N + 1)
    assert list(fused["dirichlet_slices"]) == [0, 1] and list(fused["facet_slices"]) == [0, 1]
    # Dirichlet rows: stores
    for r in (fused, two):
        assert np.array_equal(r["F"][dofs], U1.ravel()[dofs] - vals)
        assert np.array_equal(r["F_fj"][dofs], U1.ravel()[dofs] - vals)
        assert np.array_equal(r["J"][dofs], np.eye(r["J"].shape[0])[dofs])
    assert np.array_equal(fused["F"][dofs], two["F"][dofs]) and np.array_equal(fused["J"][dofs], two["J"][dofs])
    assert np.isfinite(fused["J"]).all() and np.isfinite(fused["F"]).all()
    assert eF < 1e-11 and eFJ < 1e-11, (case, eF, eFJ)
    assert eJ < 1e-10, (case, eJ)


if __name__ == "__main__":
    assert os.environ.get("FEDM_FUSED_BOUNDARY") == "0"
    mesh_, U1_, U0_ = _mesh_and_states()
    arrays = {}
    for name, deck_ in DECKS.items():
        for k, v in _assemble(mesh_, U1_, U0_, deck_).items():
            arrays[f"{name}_{k}"] = v
    np.savez(sys.argv[1], **arrays)
