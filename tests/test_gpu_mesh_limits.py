"""The patch assembly on the limit meshes of tests/limit_meshes.py against the oracle (oracle/streamer.py), for every
assembly path: the residual-only kernel, the first F + J (every plane written), a second F + J at a new state (the
constant planes kept from the first) and the product J x.  Every case asserts which kernel ran
(DeviceProblem.launched_assembly) against the kernel the band and the LDS sums of the mesh call for, and that
fedm_pattern_info predicted it.

Tolerances as in test_gpu_unstructured.py: F to 1e-11 of the per-component scale, J to 1e-10 row-relative, the
product to 1e-11.  test_mesh_limits.py shows that the oracle with one cell of the largest patch left out misses
these bounds by more than 100x: a kernel that drops a cell cannot pass.

The field split's tile sweeps on the meshes of width 12 (the widest tile instances) and beyond (no tiles): tiled
against one launch per sweep, bit for bit.  FEDM_LEAN3_CLASSES is read once per process: a child process."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))
import limit_meshes as lm  # noqa: E402
from test_gpu_unstructured import _developed_state, _rel_rows  # noqa: E402

pytestmark = pytest.mark.gpu

DT, DT_OLD = 5e-12, 4e-12
# the assembly paths: environment read when the context is created (FEDM_LEAN3_SIG: when its plan is built, at the
# first assembly; FEDM_LEAN3_PERSISTENT: per launch)
PATHS = {
    "default": {},
    "runtime-structure": {"FEDM_LEAN3_SIG": "0"},
    "row-phase": {"FEDM_ASSEMBLY_LEAN": "2"},
    "unrolled": {"FEDM_ASSEMBLY_LEAN": "0"},
    "colour": {"FEDM_ASSEMBLY": "colour"},
    "persistent": {"FEDM_LEAN3_PERSISTENT": "1"},
}
LIMIT = 160 * 1024


class _Mesh:
    def __init__(self, coords):
        self.coords = coords


_REF = {}


def _reference(name):
    """Mesh, its pattern statistics, two developed states and the oracle's F, J at both (cached per mesh)."""
    if name not in _REF:
        from fedm_amd.device import pattern_stats
        from oracle import streamer as ost
        from oracle.mesh import Mesh as OMesh
        coords, cells = lm.build(name)
        om = ost.build(OMesh(coords, cells))
        U, Uo, Uo1 = _developed_state(_Mesh(coords), 11)
        U2 = U + 0.05 * np.random.default_rng(3).standard_normal(U.shape)
        ref1 = om.residual_jacobian(U, Uo, Uo1, DT, DT_OLD)
        ref2 = om.residual_jacobian(U2, Uo, Uo1, DT, DT_OLD)
        _REF[name] = (coords, cells, pattern_stats(coords, cells, reorder=False), (U, Uo, Uo1, U2), ref1, ref2)
    return _REF[name]


def expected_kernel(stats, env, jacobian, first):
    """(variant, threads) the dispatch must take: assemble.hip assembly_path / context.cpp's choice of the colouring,
    restated from the mesh's statistics and the LDS sums (limit_meshes.lds_bytes)."""
    cells, w, v = stats["max_patch_cells"], stats["max_patch_width"], stats["max_patch_verts"]
    lds = lm.lds_bytes(w, v)
    if env.get("FEDM_ASSEMBLY") == "colour" or v > 255 or lds["generic"] > LIMIT:
        return "global colouring", 256
    lean = {"0": 0, "3": 3}.get(env.get("FEDM_ASSEMBLY_LEAN", "3")[0], 2)
    lean3_lds = (lds["lean3_all_planes"] if first else lds["lean3_planes_kept"]) if jacobian else 8 * (192 + 9 * v)
    if lean >= 3 and cells <= 384 and lean3_lds <= LIMIT:
        return "lds-patches/one-pass", 192
    if lean >= 2 and cells <= 256:
        return "lds-patches", 192 if cells <= 192 else 256
    return "lds-patches/unrolled", 192 if cells <= 192 else 320


def _run(name, env):
    """The four comparisons on one context; returns the errors and what ran."""
    coords, cells, stats, (U, Uo, Uo1, U2), (F1, J1), (F2, J2) = _reference(name)
    prob = lm.device_problem(coords, cells)
    out = dict(predicted=[], launched=[])
    try:
        prob.set_state(U, Uo, Uo1)
        prob.set_step(DT, DT_OLD)
        scale = np.abs(F1).reshape(-1, 3).max(axis=0)
        F, _ = prob.residual()
        out["launched"].append(prob.launched_assembly()["residual"])
        out["F_residual"] = float((np.abs(F - F1).reshape(-1, 3) / scale).max())
        sz = prob.sizes()
        out["predicted"].append((sz["assembly_variant"], sz["patch_threads"]))
        prob.jacobian()
        out["launched"].append(prob.launched_assembly()["jacobian"])
        out["F_first"] = float((np.abs(prob.residual_vector() - F1).reshape(-1, 3) / scale).max())
        J = prob.jacobian_csr()
        out["J_first"] = float(_rel_rows(J, J1))
        x = np.random.default_rng(5).normal(size=prob.n)
        y, yc = prob.spmv(x), J1 @ x
        out["product"] = float(np.abs(y - yc).max() / np.abs(yc).max())
        sz = prob.sizes()
        out["predicted"].append((sz["assembly_variant"], sz["patch_threads"]))
        prob.set_state(U2, Uo, Uo1)
        prob.jacobian()
        out["launched"].append(prob.launched_assembly()["jacobian"])
        scale2 = np.abs(F2).reshape(-1, 3).max(axis=0)
        out["F_second"] = float((np.abs(prob.residual_vector() - F2).reshape(-1, 3) / scale2).max())
        out["J_second"] = float(_rel_rows(prob.jacobian_csr(), J2))
        out["n_slices"] = prob.sizes()["n_slices"]
    finally:
        prob.close()
    return out


def _check(name, env, r, persistent=False, classes=False):
    stats = _reference(name)[2]
    want = [expected_kernel(stats, env, False, True), expected_kernel(stats, env, True, True),
            expected_kernel(stats, env, True, False)]
    ran = [(x["variant"], x["threads"]) for x in r["launched"]]
    assert ran == want, (name, env, ran, want)
    # fedm_pattern_info predicts the next Jacobian's kernel (before the first one: all planes written)
    assert [tuple(p) for p in r["predicted"]] == want[1:], (name, env, r["predicted"], want[1:])
    for what, x in zip(("residual", "first", "second"), r["launched"]):
        if x["variant"] == "lds-patches/one-pass" and persistent:
            # as many workgroups as the chip holds (a multiple of 8: more than the patches of a small mesh), each
            # taking its patches one after the other
            assert x["launches"] == 1 and x["workgroups"] <= max(8, r["n_slices"]), (name, what, x)
        elif x["variant"] == "lds-patches/one-pass" and classes and what == "second":
            assert x["launches"] in (1, 2) and x["workgroups"] == r["n_slices"], (name, what, x)
        elif x["variant"] != "global colouring":
            assert x["launches"] == 1 and x["workgroups"] == r["n_slices"], (name, what, x)
    for k in ("F_residual", "F_first", "F_second"):
        assert r[k] < 1e-11, (name, env, k, r[k])
    for k in ("J_first", "J_second"):
        assert r[k] < 1e-10, (name, env, k, r[k])
    assert r["product"] < 1e-11, (name, env, r["product"])


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", lm.NAMES)
def test_assembly_against_the_oracle(name, path, monkeypatch):
    env = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(name, env, _run(name, env), persistent=path == "persistent")


def test_the_refused_one_pass_jacobian_does_not_drop_cells():
    """cells384-refused: the first Jacobian does not fit the one-pass kernel's LDS (nine planes), the later ones do.
    Patches of up to 277 cells: the first one goes to the generic kernel that loops over the cells (the row-phase
    kernel takes 256 of them), the second to the one-pass kernel -- which keeps the potential plane the first wrote."""
    r = _run("cells384-refused", {})
    assert [x["variant"] for x in r["launched"]] == ["lds-patches/one-pass", "lds-patches/unrolled",
                                                      "lds-patches/one-pass"], r["launched"]
    assert r["launched"][1]["threads"] == 320
    _check("cells384-refused", {}, r)


# ---- FEDM_LEAN3_CLASSES (read once per process): a child process --------------------------------------------------
CLASS_MESHES = ("cells256", "cells384", "cells384-refused", "verts255", "width12")


def test_assembly_with_the_patch_classes(tmp_path):
    """FEDM_LEAN3_CLASSES=1: the Jacobians with the planes kept in two launches where most patches fit a quarter of
    the CU's LDS and a few do not, each sized for its class."""
    out = tmp_path / "classes.json"
    e = dict(os.environ, FEDM_LEAN3_CLASSES="1", PYTHONPATH=os.pathsep.join([str(ROOT), str(HERE)]))
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "classes", str(out)], env=e, cwd=str(ROOT),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    for name, r in json.loads(out.read_text()).items():
        _check(name, {}, r, classes=True)


# ---- tile sweeps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["width12", "width13+"])
def test_tiled_sweeps_equal_the_sweeps_one_by_one(name):
    """The species sweeps and the multigrid's finest level on tiles (the <..., 12> instances at width 12; none
    beyond: the sweeps one launch each) against one launch per sweep, bit for bit."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights, fieldsplit_tiles_stats
    coords, cells = lm.build(name)
    width = fieldsplit_tiles_stats(coords, cells, reorder=False)["row_width"]
    prob = lm.device_problem(coords, cells)
    U, Uo, Uo1 = _developed_state(_Mesh(coords), 5)
    prob.set_state(U, Uo, Uo1)
    prob.set_step(DT, DT_OLD)
    prob.setup_multigrid(**streamer.MULTIGRID)
    prob.set_fieldsplit(chebyshev_weights(6))
    prob.jacobian()
    t = np.random.default_rng(1).standard_normal(prob.n)
    prob.configure_fieldsplit_tiles(False)
    assert prob.fieldsplit_tiles() is None
    z_ref = prob.fieldsplit_apply(t)
    assert np.isfinite(z_ref).all() and np.abs(z_ref).max() > 0
    prob.configure_fieldsplit_tiles(True, multigrid=False)
    info = prob.fieldsplit_tiles()
    if width <= 12:
        assert width >= 10 and info is not None and info["row_width"] == width, (width, info)
    else:
        assert info is None, (width, info)
    assert np.array_equal(prob.fieldsplit_apply(t), z_ref)
    # the polynomial smoother's finest-level sweeps on the same tiles: the species part bit for bit
    prob.setup_multigrid(nu=1, omega=0.85, poly_degree=2)
    prob.jacobian()
    prob.configure_fieldsplit_tiles(True, multigrid=False)
    z0 = prob.fieldsplit_apply(t).reshape(-1, 3)
    prob.configure_fieldsplit_tiles(True, multigrid=True)
    z1 = prob.fieldsplit_apply(t).reshape(-1, 3)
    prob.close()
    assert np.array_equal(z1[:, :2], z0[:, :2])
    assert np.abs(z1[:, 2] - z0[:, 2]).max() <= 1e-5 * np.abs(z0[:, 2]).max()


if __name__ == "__main__":
    job, path = sys.argv[1], sys.argv[2]
    assert job == "classes"
    Path(path).write_text(json.dumps({n: _run(n, {}) for n in CLASS_MESHES}))
