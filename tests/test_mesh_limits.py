"""The limit meshes of tests/limit_meshes.py land in their bands (the library's pattern_stats, no GPU), on the intended
side of the LDS limits that choose the assembly kernel, and the bounds of test_gpu_mesh_limits.py can see a dropped
cell."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import limit_meshes as lm  # noqa: E402

KIB64, KIB160 = 64 * 1024, 160 * 1024


@pytest.fixture(scope="module")
def stats():
    from fedm_amd.device import pattern_stats
    return {n: pattern_stats(*lm.build(n), reorder=False) for n in lm.NAMES}


def _lean2_lds(width, verts, threads):
    """assemble.hip assemble_patch_t, the row-phase kernels: one row of accumulators (64 w 3), the residual (64 x 3),
    the staged vertex data (coordinates 2 v, u 3 v, folded history 2 v, exp(u / 6) 2 v) and the column of cell
    constants, LeanStash<1>::N = 5 + 2 doubles a thread (element_lean.hpp:41)."""
    return 8 * (64 * 3 * width + 64 * 3 + 2 * verts + (3 + 2 * 2) * verts + 7 * threads)


def test_the_meshes_are_conforming_triangulations_of_the_domain():
    for name in lm.NAMES:
        coords, cells = lm.build(name)
        assert coords.min() == 0.0 and coords.max() == lm.BOX, name
        p = coords[cells]
        det = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
        assert (det > 0).all(), name
        assert 0.5 * det.sum() == pytest.approx(lm.BOX ** 2, rel=1e-12), name
        # every edge has one cell on either side, or lies on the boundary
        e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]]), axis=1)
        _, counts = np.unique(e, axis=0, return_counts=True)
        assert counts.max() == 2, name
        used = np.zeros(coords.shape[0], bool)
        used[cells] = True
        assert used.all(), name


def test_each_mesh_lands_in_its_band(stats):
    c = {n: s["max_patch_cells"] for n, s in stats.items()}
    w = {n: s["max_patch_width"] for n, s in stats.items()}
    v = {n: s["max_patch_verts"] for n, s in stats.items()}
    assert c["cells192"] <= 192
    for n in ("cells256", "cells256-lean2"):
        assert 193 <= c[n] <= 256, n
    for n in ("cells384", "cells384-refused"):
        assert 257 <= c[n] <= 384, n
    assert c["cells384"] == 384                        # every thread of 192 takes a second cell
    assert c["cells385+"] > 384 and v["cells385+"] <= 255
    assert v["colour-verts"] > 255
    assert v["verts255"] == 255
    assert 10 <= w["width12"] <= 12
    assert w["width13+"] > 12
    assert stats["small"]["n_slices"] < 8 and lm.build("small")[0].shape[0] % 64 != 0
    # no wheel where none is wanted
    for n in ("cells192", "cells256", "cells384", "colour-verts", "verts255", "small"):
        assert w[n] <= 9, n
    for n in lm.NAMES:
        if n != "colour-verts":
            assert v[n] <= 255, n


def test_the_lds_sums_put_each_mesh_on_its_side_of_the_limits(stats):
    """Dynamic LDS of one workgroup (limit_meshes.lds_bytes restates assemble3.hip lean3_lds_bytes and assemble.hip
    patch_lds_bytes): a one-pass launch beyond 160 KiB is refused (assemble3.hip lean3_fits), beyond it the LDS patches
    are given up for the global colouring (context.cpp fedm_ctx_create), and beyond 64 KiB a launch needs more than the
    default dynamic LDS."""
    lds = {n: lm.lds_bytes(s["max_patch_width"], s["max_patch_verts"]) for n, s in stats.items()}
    for n in ("cells192", "cells256", "cells384", "verts255", "small"):
        assert lds[n]["lean3_all_planes"] <= KIB64 and lds[n]["generic"] <= KIB64, n
    # the row-phase kernels with more than 64 KiB where the one-pass first Jacobian is refused
    n = "cells256-lean2"
    assert lds[n]["lean3_all_planes"] > KIB160 and lds[n]["lean3_planes_kept"] <= KIB160 and lds[n]["generic"] <= KIB160
    assert _lean2_lds(stats[n]["max_patch_width"], stats[n]["max_patch_verts"], 256) > KIB64
    # refused on the first Jacobian, fitting afterwards, patches beyond 256 cells: the row-phase kernels must not run
    n = "cells384-refused"
    assert lds[n]["lean3_all_planes"] > KIB160 and lds[n]["lean3_planes_kept"] <= KIB160 and lds[n]["generic"] <= KIB160
    assert lds[n]["generic"] > KIB64
    # the generic kernel beyond 64 KiB, looping over more than 384 cells
    assert KIB64 < lds["cells385+"]["generic"] <= KIB160
    assert lds["colour-lds"]["generic"] > KIB160
    for n in ("width12", "width13+"):
        assert KIB64 < lds[n]["lean3_all_planes"] <= KIB160, n


@pytest.mark.parametrize("name", ["cells384-refused", "cells385+", "cells384"])
def test_the_bounds_see_a_dropped_cell(name):
    """The oracle's F and J with one cell of the largest patch left out miss test_gpu_mesh_limits.py's bounds (F 1e-11
    of the component scale, J 1e-10 row-relative) by more than 100x."""
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from test_gpu_mesh_limits import DT, DT_OLD, _Mesh, _developed_state, _rel_rows
    coords, cells = lm.build(name)
    sl = cells // 64
    per_slice = np.array([np.count_nonzero((sl == s).any(axis=1)) for s in range(sl.max() + 1)])
    patch = np.flatnonzero((sl == per_slice.argmax()).any(axis=1))
    U, Uo, Uo1 = _developed_state(_Mesh(coords), 11)
    F, J = ost.build(OMesh(coords, cells)).residual_jacobian(U, Uo, Uo1, DT, DT_OLD)
    Fd, Jd = ost.build(OMesh(coords, np.delete(cells, patch[-1], axis=0))).residual_jacobian(U, Uo, Uo1, DT, DT_OLD)
    scale = np.abs(F).reshape(-1, 3).max(axis=0)
    assert (np.abs(Fd - F).reshape(-1, 3) / scale).max() > 100 * 1e-11
    assert _rel_rows(Jd, J) > 100 * 1e-10
