"""Host side of the field output (csrc/fields.hip; ``DeviceProblem.fields_setup`` / ``probe_setup`` / ``fields``):
the P1 mass matrix of the plain measure, point location for the probes, and the field names of the facade.

Nothing here touches the device; tests/test_field_output_reference.py pins the point location on closed forms.
"""
import numpy as np

KINDS = {"state": 0, "density": 1, "charge": 2, "e_r": 3, "e_z": 4, "e_norm": 5, "rate": 6, "flux_r": 7, "flux_z": 8}
INDEXED = {"state", "density", "rate", "flux_r", "flux_z"}
PROJECTED = {"e_r", "e_z", "e_norm", "rate", "flux_r", "flux_z"}
MAX_REQUESTS = 8
# the LMEA family's kinds (include/fedm_hip.h, FEDM_GD_FIELD_*): component 0 is the energy, species 0 the gas
GD_KINDS = {"state": 32, "density": 33, "charge": 34, "mean_energy": 35, "table": 36, "e_r": 37, "e_z": 38, "e_norm": 39,
            "reduced_field": 40, "rate": 41, "source": 42, "collision_loss": 43, "joule": 44, "flux_r": 45, "flux_z": 46,
            "current_r": 47, "current_z": 48}
GD_INDEXED = {"state", "density", "table", "rate", "source", "flux_r", "flux_z"}
GD_BY_SPECIES = {"density", "source", "flux_r", "flux_z"}          # their index may be a species name
GD_POTENTIAL_ONLY = {"e_r", "e_z", "e_norm", "reduced_field"}
# evaluated as the residual of the current step evaluates them (u_new, the field table as it stands): no blend
GD_OF_THE_STEP = {"table", "rate", "source", "collision_loss", "joule", "flux_r", "flux_z", "current_r", "current_z"}
GD_PROJECTED = GD_POTENTIAL_ONLY | (GD_OF_THE_STEP - {"table"})


def mass_matrix(coords, cells):
    """The consistent P1 mass matrix of the plain measure ``dx``: ``|det J| / 24 (1 + delta_ab)`` per cell (CSR)."""
    import scipy.sparse as sp
    x = coords[cells]
    d1, d2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    det = np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
    vals = det[:, None, None] * ((np.ones((3, 3)) + np.eye(3)) / 24.0)[None]
    c = cells.astype(np.int64)
    rows = np.broadcast_to(c[:, :, None], vals.shape).ravel()
    cols = np.broadcast_to(c[:, None, :], vals.shape).ravel()
    n = coords.shape[0]
    M = sp.coo_matrix((vals.ravel(), (rows, cols)), shape=(n, n)).tocsr()
    M.sort_indices()
    return M


def locate_points(coords, cells, points, tol=1e-12, chunk=4_000_000):
    """``(cell[n], weights[n, 3])``: the cell that contains each point and the point's barycentric weights there.
    A point on an edge or a vertex belongs to several cells: the lowest cell index takes it.  ``tol``: how far below 0
    a barycentric weight may lie (a point on the boundary, up to rounding).  A point in no cell raises ``ValueError``
    naming it.  Vectorised over (points, cells) in chunks of ``chunk`` pairs."""
    coords = np.asarray(coords, dtype=np.float64)
    cells = np.asarray(cells)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    # only the cells whose bounding box meets the points' (an axis profile looks at the cells along the axis); their
    # indices stay in ascending order, so the lowest index still wins
    xc = coords[cells]
    pad = 1e-9 * float(np.abs(coords).max()) if coords.size else 0.0
    near = np.ones(cells.shape[0], dtype=bool)
    if pts.shape[0]:
        near = ((xc.min(axis=1) <= pts.max(axis=0) + pad) & (xc.max(axis=1) >= pts.min(axis=0) - pad)).all(axis=1)
    keep = np.nonzero(near)[0]
    x0, x1, x2 = xc[keep, 0], xc[keep, 1], xc[keep, 2]
    e1, e2 = x1 - x0, x2 - x0
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    nc = keep.size
    found = np.empty(pts.shape[0], dtype=np.int64)
    w = np.empty((pts.shape[0], 3))
    step = max(1, chunk // max(nc, 1))
    for lo in range(0, pts.shape[0], step):
        p = pts[lo:lo + step]
        dx = p[:, None, 0] - x0[None, :, 0]
        dy = p[:, None, 1] - x0[None, :, 1]
        l1 = (dx * e2[None, :, 1] - dy * e2[None, :, 0]) / det[None, :]
        l2 = (e1[None, :, 0] * dy - e1[None, :, 1] * dx) / det[None, :]
        l0 = 1.0 - l1 - l2
        inside = np.minimum(np.minimum(l0, l1), l2) >= -tol
        hit = inside.any(axis=1) if nc else np.zeros(p.shape[0], dtype=bool)
        if not hit.all():
            k = lo + int(np.nonzero(~hit)[0][0])
            raise ValueError(f"probe point {k} at ({pts[k, 0]!r}, {pts[k, 1]!r}) lies outside the mesh")
        first = inside.argmax(axis=1)                       # the lowest cell index that holds the point
        rows = np.arange(p.shape[0])
        found[lo:lo + step] = keep[first]
        w[lo:lo + step] = np.stack([l0[rows, first], l1[rows, first], l2[rows, first]], axis=1)
    return found, w


def parse_request(name, n_species, n_eq, n_reactions, species_names=None):
    """``(kind, index)`` of a field name: ``"E_norm"``, ``"E_r"``, ``"E_z"``, ``"charge"``, ``"state:2"``,
    ``"density:1"`` or ``"density:electrons"`` (with ``species_names``), ``"rate:0"``, ``"flux_r:1"``, ``"flux_z:1"``.
    A pair ``(kind, index)`` passes through (kind a name or a number)."""
    if isinstance(name, str):
        head, _, tail = name.partition(":")
    else:
        head, tail = name[0], name[1] if len(name) > 1 else ""
    if isinstance(head, str):
        key = head.strip().lower()
        if key not in KINDS:
            raise ValueError(f"field '{name}': unknown kind '{head}' (one of {', '.join(sorted(KINDS))})")
    else:
        key = next((k for k, v in KINDS.items() if v == int(head)), None)
        if key is None:
            raise ValueError(f"field {name!r}: unknown kind {head}")
    index = 0
    if key in INDEXED:
        if tail == "" or tail is None:
            raise ValueError(f"field '{name}': '{key}' needs an index ('{key}:0')")
        names = list(species_names or ())
        if isinstance(tail, str) and tail.strip() in names and key != "rate":
            index = names.index(tail.strip())
        else:
            try:
                index = int(tail)
            except (TypeError, ValueError):
                raise ValueError(f"field '{name}': '{tail}' is neither an index nor one of the species {names}") from None
        limit = {"state": n_eq, "rate": n_reactions}.get(key, n_species)
        if not 0 <= index < limit:
            raise ValueError(f"field '{name}': index {index} out of range (0 to {limit - 1})")
    elif tail not in ("", None):
        raise ValueError(f"field '{name}': '{key}' takes no index")
    return KINDS[key], index


def gd_kind_name(request):
    """The kind of a request of :func:`parse_gd_request` as a lower-case name (``"rate"`` of ``"rate:3"``)."""
    head = request.partition(":")[0] if isinstance(request, str) else request[0]
    if isinstance(head, str):
        return head.strip().lower()
    return next((k for k, v in GD_KINDS.items() if v == int(head)), None)


def parse_gd_request(name, n_species, n_reactions, n_fields, species_names=None):
    """``(kind, index)`` of a field name of the LMEA family: ``"state:e"``, ``"density:s"``, ``"charge"``,
    ``"mean_energy"``, ``"table:f"``, ``"E_r"``, ``"E_z"``, ``"E_norm"``, ``"reduced_field"``, ``"rate:j"``, ``"source:s"``,
    ``"collision_loss"``, ``"joule"``, ``"flux_r:s"``, ``"flux_z:s"``, ``"current_r"``, ``"current_z"``.  ``s`` is an index
    or one of ``species_names`` (the gas is index 0; component 0 is the energy: ``"density:0"`` is the energy density and
    ``"flux_z:0"`` the energy flux; ``"source"`` starts at 1).  A pair ``(kind, index)`` passes through (kind a name or a
    number)."""
    if isinstance(name, str):
        head, _, tail = name.partition(":")
    else:
        head, tail = name[0], name[1] if len(name) > 1 else ""
    key = gd_kind_name(name)
    if key not in GD_KINDS:
        raise ValueError(f"field {name!r}: unknown kind {head!r} (one of {', '.join(sorted(GD_KINDS))})")
    index = 0
    if key in GD_INDEXED:
        if tail == "" or tail is None:
            raise ValueError(f"field '{name}': '{key}' needs an index ('{key}:1')")
        names = list(species_names or ())
        if isinstance(tail, str) and tail.strip() in names and key in GD_BY_SPECIES:
            index = names.index(tail.strip())
        else:
            try:
                index = int(tail)
            except (TypeError, ValueError):
                raise ValueError(f"field '{name}': '{tail}' is neither an index nor one of the species {names}") from None
        first = 1 if key == "source" else 0
        limit = {"state": n_species + 1, "rate": n_reactions, "table": n_fields}.get(key, n_species)
        if not first <= index < limit:
            raise ValueError(f"field '{name}': index {index} out of range ({first} to {limit - 1})")
    elif tail not in ("", None):
        raise ValueError(f"field '{name}': '{key}' takes no index")
    return GD_KINDS[key], index
