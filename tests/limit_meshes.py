"""Meshes of the streamer domain [0, BOX]^2 at the limits of the patch assembly and the field split's tile sweeps
(helper module of test_mesh_limits.py and test_gpu_mesh_limits.py).

The assembly kernels and the tile sweeps are chosen from three statistics of a mesh's 64-vertex slices: the cells of
a patch (every cell that touches one of the slice's vertices), the ELL width of a slice (largest valence + 1) and the
staged vertices of a patch (the slice and its halo).  The device numbering is the builder's (``DeviceProblem(...,
reorder=False)``: `device_problem`), so each mesh puts its patches where it wants them:

* a grid numbered row by row: a slice is a run of 64 consecutive vertices, so 32 columns give two rows a slice and
  186 cells a patch, 64 columns one row and 252 cells, 100 columns runs that straddle two rows and up to 260 cells;
* a wheel of K spokes -- a centre vertex joined to the K vertices of a rectangle of grid points around it, whose
  inner grid points are removed -- gives width K + 1 to the slice of its centre;
* a slice made of vertices that share no edge (the grid points with i + j = 0 mod 3) puts its halo vertices inside
  the patch: 64 x 6 cells, about 170 halo vertices; with a wheel centre among them the patch has more cells than
  the 384 the one-pass kernels take, and spread out over the mesh they stage more vertices;
* a scrambled numbering gives more than 255 staged vertices.

Every triangle is explicit (no Delaunay, nothing left to a library's choice between cocircular points).  Each mesh
is named after its band, which test_mesh_limits.py checks with the library's ``pattern_stats``; `lds_bytes` restates
the sums of LDS bytes that decide between the kernels.

Contiguous row runs keep every halo vertex on the patch's rim (cells = 2 V - B - 2 for V vertices, B of them on the
rim: at most 126 + h cells for h halo vertices); the interleaved slices reach beyond 384 cells with ``patch_ok``
(`cells385+`: 390 cells, 235 staged vertices)."""
import numpy as np

BOX = 0.0125          # fedm_amd.cases.streamer.BOX


class _Grid:
    """(nx x ny) grid of [0, BOX]^2, vertex (i, j) = j nx + i, quads split along their rising diagonal; wheels
    replace the cells inside a rectangle of grid lines by a fan around one grid point."""

    def __init__(self, nx, ny):
        self.nx, self.ny = nx, ny
        x, y = np.meshgrid(np.linspace(0.0, BOX, nx), np.linspace(0.0, BOX, ny))
        self.coords = np.column_stack([x.ravel(), y.ravel()])
        i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1))
        a = (j * nx + i).ravel()
        self.cells = np.concatenate([np.column_stack([a, a + 1, a + nx + 1]), np.column_stack([a, a + nx + 1, a + nx])])
        self.alive = np.ones(nx * ny, bool)

    def vid(self, i, j):
        return j * self.nx + i

    def wheel(self, i0, j0, a1, a2, b1, b2, skip=0):
        """Centre (i0, j0), rectangle [i0 - a1, i0 + a2] x [j0 - b1, j0 + b2]: 2 (a1 + a2 + b1 + b2) - skip spokes
        (`skip` of the rectangle's corners are cut off by a triangle of their two ring neighbours)."""
        nx = self.nx
        lo_i, hi_i, lo_j, hi_j = i0 - a1, i0 + a2, j0 - b1, j0 + b2
        assert 0 < lo_i and hi_i < nx - 1 and 0 < lo_j and hi_j < self.ny - 1 and min(a1, a2, b1, b2) >= 1
        ci, cj = self.cells % nx, self.cells // nx
        inside = ((ci >= lo_i) & (ci <= hi_i) & (cj >= lo_j) & (cj <= hi_j)).all(axis=1)
        self.cells = self.cells[~inside]
        for j in range(lo_j + 1, hi_j):
            for i in range(lo_i + 1, hi_i):
                if (i, j) != (i0, j0):
                    self.alive[self.vid(i, j)] = False
        # the ring counter-clockwise from the lower left corner
        ring = ([(i, lo_j) for i in range(lo_i, hi_i)] + [(hi_i, j) for j in range(lo_j, hi_j)] +
                [(i, hi_j) for i in range(hi_i, lo_i, -1)] + [(lo_i, j) for j in range(hi_j, lo_j, -1)])
        corners = [(lo_i, lo_j), (hi_i, lo_j), (hi_i, hi_j), (lo_i, hi_j)][:skip]
        ring = [self.vid(*p) for p in ring]
        cut = {self.vid(*p) for p in corners}
        c = self.vid(i0, j0)
        spokes = [r for r in ring if r not in cut]
        new = [[c, spokes[k], spokes[(k + 1) % len(spokes)]] for k in range(len(spokes))]
        for k, r in enumerate(ring):
            if r in cut:
                new.append([ring[k - 1], r, ring[(k + 1) % len(ring)]])
        self.cells = np.vstack([self.cells, np.array(new)])
        return len(spokes)

    def mesh(self, first=()):
        """(coords, cells) numbered row by row, the vertices of `first` (grid ids) ahead of all others."""
        first = np.asarray(first, dtype=np.int64)
        rest = np.flatnonzero(self.alive)
        rest = rest[~np.isin(rest, first)]
        order = np.concatenate([first, rest])
        inv = np.full(self.coords.shape[0], -1, dtype=np.int64)
        inv[order] = np.arange(order.size)
        cells = inv[self.cells]
        assert (cells >= 0).all()
        return _ccw(self.coords[order], cells)

    def sublattice(self, i0, j0, n, exclude=()):
        """n grid points with i + j = 0 mod 3 (no two of them share an edge), the nearest ones to (i0, j0)."""
        i, j = np.meshgrid(np.arange(1, self.nx - 1), np.arange(1, self.ny - 1))
        i, j = i.ravel(), j.ravel()
        ok = ((i + j) % 3 == 0) & self.alive[self.vid(i, j)] & ~np.isin(self.vid(i, j), list(exclude))
        i, j = i[ok], j[ok]
        d = (i - i0) ** 2 + (j - j0) ** 2 + 1e-3 * (j * self.nx + i) / (self.nx * self.ny)
        k = np.argsort(d)[:n]
        return self.vid(i[k], j[k])


def _ccw(coords, cells):
    p = coords[cells]
    det = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    assert (np.abs(det) > 0).all()
    cells = cells.copy()
    cells[det < 0] = cells[det < 0][:, [0, 2, 1]]
    return np.ascontiguousarray(coords), np.ascontiguousarray(cells, dtype=np.int32)


def _ring(nx, ny, spokes_rect, skip, centre, first=None):
    g = _Grid(nx, ny)
    g.wheel(*centre, *spokes_rect, skip=skip)
    return g.mesh() if first is None else g.mesh(first(g))


def build(name):
    """(coords, cells) of the named limit mesh."""
    if name == "cells192":        # two rows of 32 a slice: 186 cells, width 7 (20 slices)
        return _Grid(32, 40).mesh()
    if name == "cells256":        # one row of 64 a slice: 252 cells, width 7; lean3 fits (19 slices)
        return _Grid(64, 19).mesh()
    if name == "cells256-lean2":  # 40 columns, a wheel of 32 spokes: width 33
        return _ring(40, 40, (4, 4, 4, 4), 0, (20, 20))
    if name == "cells384":        # one slice of 64 pairwise non-adjacent vertices: 384 cells
        g = _Grid(32, 40)
        return g.mesh(g.sublattice(16, 20, 64))
    if name == "cells384-refused":  # 100 columns (up to 260 cells), a wheel of 31 spokes: width 32
        return _ring(100, 30, (4, 4, 4, 4), 1, (50, 15))
    if name == "cells385+":       # the interleaved slice around the centre of a wheel of 12 spokes: 390 cells
        g = _Grid(40, 40)
        g.wheel(20, 19, 2, 2, 1, 1)
        c = g.vid(20, 19)
        return g.mesh(np.concatenate([[c], g.sublattice(20, 19, 63, exclude=_ring_ids(g, 20, 19, 2, 2, 1, 1))]))
    if name == "colour-lds":      # a wheel of 34 spokes: width 35, the generic patch kernel's LDS over 160 KiB
        return _ring(40, 40, (4, 4, 4, 5), 0, (20, 20))
    if name == "colour-verts":    # a scrambled numbering: every slice stages ~ 300 vertices
        coords, cells = _Grid(32, 32).mesh()
        order = np.random.default_rng(7).permutation(coords.shape[0])
        inv = np.empty_like(order)
        inv[order] = np.arange(order.size)
        return _ccw(coords[order], inv[cells])
    if name == "verts255":        # the interleaved slice spread until it stages exactly 255 vertices
        g = _Grid(40, 40)
        return g.mesh(_spread_sublattice(g, 191))
    if name == "width12":         # a wheel of 11 spokes: width 12
        return _ring(32, 40, (1, 2, 1, 2), 1, (16, 20))
    if name == "width13+":        # a wheel of 14 spokes: width 15
        return _ring(32, 40, (2, 2, 2, 1), 0, (16, 20))
    if name == "small":           # 17 x 17: five slices, the last one of 33 vertices
        return _Grid(17, 17).mesh()
    raise KeyError(name)


def _ring_ids(g, i0, j0, a1, a2, b1, b2):
    return [g.vid(i, j) for j in range(j0 - b1, j0 + b2 + 1) for i in range(i0 - a1, i0 + a2 + 1)]


def _spread_sublattice(g, target_halo):
    """64 pairwise non-adjacent grid points whose neighbours number exactly `target_halo`: a compact block of them
    with the last ones moved, one at a time, to isolated places (each of those stages its six neighbours alone)."""
    nbr = {}
    for a, b, c in g.cells:
        for p, q in ((a, b), (b, c), (c, a)):
            nbr.setdefault(p, set()).add(q)
            nbr.setdefault(q, set()).add(p)
    block = list(g.sublattice(10, 10, 64))
    far = [v for v in g.sublattice(30, 30, 400) if v not in block]
    halo = lambda S: len(set().union(*(nbr[v] for v in S)) - set(S))
    S = list(block)
    k = 0
    while halo(S) < target_halo:
        S.pop(len(S) - 1 - 0)
        # an isolated place: no neighbour shared with what is taken
        taken = set().union(*(nbr[v] for v in S))
        while nbr[far[k]] & taken:
            k += 1
        S.insert(0, far[k])
        k += 1
        if halo(S) > target_halo:
            # overshot by moving a whole vertex: put it next to the block instead (shares neighbours with it)
            S.pop(0)
            for v in g.sublattice(10, 10, 200):
                if v in S:
                    continue
                T = [v] + S
                if halo(T) == target_halo:
                    return T
            raise AssertionError("no placement stages exactly the target")
    return S


NAMES = ("cells192", "cells256", "cells256-lean2", "cells384", "cells384-refused", "cells385+", "colour-lds",
         "colour-verts", "verts255", "width12", "width13+", "small")


def device_problem(coords, cells, **kw):
    """The streamer model on a limit mesh, in the builder's numbering (tags and Dirichlet data as the deck's)."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem
    from fedm_amd.mesh import Marking_boundaries, Mesh
    msh = Mesh(coords, cells)
    assert np.array_equal(msh.coords, coords) and np.array_equal(msh.cells, cells)
    dofs, vals = streamer.dirichlet(msh.coords)
    return DeviceProblem(msh.coords, msh.cells, streamer.model(), facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                         dirichlet_dofs=dofs, dirichlet_vals=vals, reorder=False, **kw)


def lds_bytes(width, verts):
    """Dynamic LDS of one patch workgroup for the widest slice (`width` block columns) and the most staged vertices
    (`verts`), streamer model (two species + potential: 3 equations, 9 planes):

    * one-pass kernels, all nine planes (first Jacobian):  8 (64 w 9 + 64 * 3 + 2 v + (3 + 2 * 2) v)
    * one-pass kernels, the potential plane kept (eight):  8 (64 w 8 + 64 * 3 + 9 v)
      (assemble3.hip, lean3_lds_bytes: acc + SLICE neq + 2 verts + (neq + 2 ns) verts doubles)
    * generic patch kernel:                                8 (64 w 9 + 64 * 3 + 2 v + (3 + 2) v)
      (assemble.hip, patch_lds_bytes: acc + SLICE neq + 2 mv + (neq + ns) mv doubles)"""
    return {"lean3_all_planes": 4608 * width + 1536 + 72 * verts,
            "lean3_planes_kept": 4096 * width + 1536 + 72 * verts,
            "generic": 4608 * width + 1536 + 56 * verts}
