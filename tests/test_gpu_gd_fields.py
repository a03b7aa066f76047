"""The LMEA field output on the device (csrc/gd_fields.hip, DeviceProblem.gd_fields) against the numpy restatement of
tests/gd_fields_reference.py, which tests/test_gd_fields_reference.py pins on the balance's restatement and on closed
forms; against the device's own balance; and against the refresh pipeline's reduced field.

Models of tests/lmea_models.py: e-only (3 equations), ion-e (4; grad_diffusion on and off, powers of 2),
deck-shape-permuted (5; a 'reaction' species whose flux is 0, both sentinel losses, a power of 4), two-ions-small
axisymmetric and planar (6), two-ions-full (6; all 16 rates over two calls).  Meshes: 3 x 3 (18 cells, less than a wave),
10 x 10 (400 cells: two workgroups, the second partly empty), irregular (1 328 cells, valence 4 to 11) for the two
models lmea_models.IRREGULAR_FOR names.

Bounds.  Projected kinds, lumped: |device - b / m| m <= 1e-12 sum|terms| at every vertex (tests/test_gpu_field_output.py's
SUM_BOUND).  Consistent at rtol 1e-10: |b - M X| <= 2 rtol |b| and |X - X_direct| <= 2 |b - M X| / min m.  Pointwise:
density and charge 4 eps sum|addends|, mean_energy 4 eps max(1, |u_0 - u_e|) value (the exponent's rounding, eps |x|, is
the exponential's relative error), state and table bitwise.  The balance, device against device: 2e-12 sum|terms| +
4 eps sum_v |b_v|.  Every figure is printed before it is asserted.

Measured on the MI355X, as fractions of these bounds: projected kinds at most 0.064 (E_r; flux_r 0.059, flux_z 0.041,
every other kind below 0.016), charge 0.32, density 0.25, mean_energy 0.21; the consistent projection's residual 3.3e-11
to 8.9e-11 of |b| and its distance from the direct solve 0.20 to 0.46 of its bound; the balance 9.2e-5; the reduced
field 0.52 of the bound from the two solves' residuals (4.7e-11 and 3.5e-15 of |b|); blend and probes 0.  The whole file
runs in about 5 s, no test above 2 s.
"""
import ctypes as C
import dataclasses
import importlib.util
import math
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gd_fields_reference as gfr  # noqa: E402
import lmea_models  # noqa: E402
from test_gd_fields_reference import GPU_CASES, projected_names  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps
SUM_BOUND, POINT_BOUND, RTOL = 1e-12, 4 * EPS, 1e-10
OLD = dict(t_out=0.0, t_old=0.0, t=1.0)          # num = 0: X(u_old) alone
BLENDABLE = ["state:1", "density:0", "charge", "mean_energy", "E_r", "E_z", "E_norm", "reduced_field"]


def _problem(c, model=None, **kw):
    from fedm_amd.device import DeviceProblem
    prob = DeviceProblem(c.mesh.coords, c.mesh.cells, c.model if model is None else model, facet_tags=c.mesh.tags,
                         dirichlet_dofs=c.dirichlet_dofs, dirichlet_vals=c.dirichlet_vals, reorder=True, **kw)
    prob.set_gd_fields(c.fields)
    prob.set_state(c.U, c.Uo, c.Uo1)
    prob.set_step(c.dt, c.dt_old)
    return prob


class Case:
    """One (model, mesh, geometry): the restatement (computed once per (state, name), never changed) and one device
    problem with the mass matrix set up."""

    def __init__(self, name, mesh_name, planar):
        self.c = lmea_models.case(name, mesh_name, planar=planar)
        self.r = gfr.of_case(self.c)
        self.prob = _problem(self.c)
        self.prob.gd_fields_setup(consistent=True)
        self._ref = {}

    def ref(self, which, name):
        if (which, name) not in self._ref:
            self._ref[which, name] = self.r.reference(self.c.U if which == "new" else self.c.Uo, name)
        return self._ref[which, name]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name, mesh_name="10x10", planar=False):
        if (name, mesh_name, planar) not in made:
            made[name, mesh_name, planar] = Case(name, mesh_name, planar)
        return made[name, mesh_name, planar]
    yield get
    for c in made.values():
        c.prob.close()


def _ratio(err, scale):
    """max err / scale, where scale > 0; where it is 0 the error must be 0 too."""
    assert np.all(err[scale == 0.0] == 0.0)
    return float((err[scale > 0.0] / scale[scale > 0.0]).max()) if (scale > 0.0).any() else 0.0


def _check(what, res, names, ref_of, U):
    """Every request of one call against the restatement; prints the worst figure per request first."""
    assert res.finite
    worst = {}
    ns = U.shape[1] - 1
    for k, name in enumerate(names):
        dev, ref = res.nodal[k], ref_of(name)
        kind = name.split(":")[0].lower()
        if isinstance(ref, gfr.Projected):
            worst[name] = _ratio(np.abs(dev - ref.b / ref.m) * ref.m, ref.abs) / SUM_BOUND
        elif kind in ("state", "table"):
            worst[name] = 0.0 if np.array_equal(dev, ref.value) else np.inf
        elif kind == "mean_energy":
            worst[name] = _ratio(np.abs(dev - ref.value), np.maximum(1.0, np.abs(U[:, 0] - U[:, ns - 1])) * ref.value) / POINT_BOUND
        else:
            worst[name] = _ratio(np.abs(dev - ref.value), ref.abs) / POINT_BOUND
    print(f"[gd fields] {what}: error / bound " + " ".join(f"{n} {v:.2e}" for n, v in worst.items()), flush=True)
    for name, v in worst.items():
        assert v <= 1.0, (what, name, v)
    return worst


def _bytes(res):
    parts = [res.nodal, res.probes, np.array([int(res.finite)]), res.cg_iterations]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts if p is not None)


def _chunks(names, n=8):
    return [names[i:i + n] for i in range(0, len(names), n)]


def _pointwise_names(md):
    ns, nf = int(md.n_species), 4 * int(md.n_species) + 2 * int(md.n_reactions) + 3
    return ([f"state:{e}" for e in range(ns + 1)] + [f"density:{c}" for c in range(ns)] + ["charge", "mean_energy"]
            + [f"table:{f}" for f in sorted({0, ns, nf // 2, nf - 3, nf - 1})])


# ---- 1: every kind against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,mesh_name,planar", GPU_CASES)
def test_every_kind_against_the_restatement(cases, name, mesh_name, planar):
    c = cases(name, mesh_name, planar)
    what = f"{name} {mesh_name}{' planar' if planar else ''}"
    for names in _chunks(projected_names(c.c.md) + _pointwise_names(c.c.md)):
        _check(what, c.prob.gd_fields(names), names, lambda n: c.ref("new", n), c.c.U)
    old = [n for n in BLENDABLE if n != "state:1"] + [f"state:{int(c.c.md.n_species)}"]
    _check(what + " state old", c.prob.gd_fields(old, **OLD), old, lambda n: c.ref("old", n), c.c.Uo)
    ie = int(c.c.md.n_species) - 1
    assert np.abs(c.ref("new", f"flux_z:{ie}").b).max() > 0.0 and np.abs(c.ref("new", "flux_z:0").b).max() > 0.0
    assert not np.array_equal(c.prob.gd_fields(["E_norm"]).nodal, c.prob.gd_fields(["E_norm"], **OLD).nodal)
    if name == "deck-shape-permuted":      # the 'reaction' species: its flux is 0 to the bit
        res = c.prob.gd_fields(["flux_r:2", "flux_z:2"])
        assert int(c.c.md.eq_type[2]) == 0 and not res.nodal.any()


def test_the_charge_leaves_component_0_out():
    """A sign for component 0, which no row of the residual reads: the charge must not read it either."""
    c = lmea_models.case("ion-e", "10x10")
    model = dataclasses.replace(c.model, sign=[1.0] + list(c.model.sign[1:]))
    prob = _problem(c, model)
    try:
        r = gfr.of_case(c, md=model.to_c())
        _check("ion-e with a sign for component 0", prob.gd_fields(["charge"]), ["charge"], lambda n: r.reference(c.U, n), c.U)
    finally:
        prob.close()


# ---- 2: the consistent projection --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mesh_name", [("two-ions-small", "10x10"), ("deck-shape-permuted", "irregular"), ("e-only", "3x3")])
def test_consistent_projection(cases, name, mesh_name):
    import scipy.sparse.linalg as spla
    c = cases(name, mesh_name)
    names = ["E_norm", "reduced_field", "rate:0", "joule", "flux_z:0", "current_z", "source:1", "mean_energy"]
    res = c.prob.gd_fields(names, projection="consistent", rtol=RTOL)
    assert res.finite
    M = c.r.mass_matrix()
    lu = spla.splu(M.tocsc())
    print(f"[gd fields] {name} {mesh_name} consistent: CG iterations {res.cg_iterations.tolist()}", flush=True)
    assert np.all(res.cg_iterations[:7] > 0) and res.cg_iterations[7] == 0
    for k, req in enumerate(names[:7]):
        ref = c.ref("new", req)
        X = res.nodal[k]
        resid, bnorm = np.linalg.norm(ref.b - M @ X), np.linalg.norm(ref.b)
        dist = np.linalg.norm(X - lu.solve(ref.b))
        print(f"[gd fields] {name} {mesh_name} consistent {req}: |b - M X| / |b| {resid / bnorm:.2e}, "
              f"|X - X_direct| / (2 |b - M X| / min m) {dist * ref.m.min() / (2 * resid):.2e}", flush=True)
        assert resid <= 2 * RTOL * bnorm, req
        assert dist <= 2 * resid / ref.m.min(), req
    _check(f"{name} {mesh_name} consistent, the pointwise request", types.SimpleNamespace(finite=True, nodal=res.nodal[7:]),
           names[7:], lambda n: c.ref("new", n), c.c.U)
    assert _bytes(c.prob.gd_fields(names, projection="consistent", rtol=RTOL)) == _bytes(res)


# ---- 3: against the balance kernel, device against device ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["two-ions-small", "e-only"])
def test_planar_fields_sum_to_the_devices_balance(cases, name):
    c = cases(name, "10x10", True)
    bal = c.prob.balance()
    nr = int(c.c.md.n_reactions)
    names = [f"rate:{j}" for j in range(nr)] + ["joule", "collision_loss"]
    want = list(bal.reaction[:nr]) + [bal.joule, bal.collision_loss]
    res = c.prob.gd_fields(names)
    assert res.finite and bal.finite
    for k, req in enumerate(names):
        ref = c.ref("new", req)
        got = math.fsum((res.nodal[k] * ref.m).tolist())
        allowed = 2e-12 * math.fsum(ref.abs.tolist()) + 4 * EPS * math.fsum(np.abs(ref.b).tolist())
        print(f"[gd fields] planar {name} {req}: fsum_v(X_v m_v) {got:.6e} balance {want[k]:.6e} |difference| / bound "
              f"{abs(got - want[k]) / allowed:.2e}", flush=True)
        assert abs(got - want[k]) <= allowed, req


# ---- 4: the reduced field against the refresh pipeline -------------------------------------------------------------------
def test_reduced_field_against_the_refresh_pipeline():
    """After one step of the device pipeline the refresh holds project(1e21 |grad Phi| / N0) of the state it started
    from, now u_old, solved to its own tolerance (gdprep.hip: rtol 1e-14, 500 steps at the most).  Both solutions'
    residuals are formed here, against the restatement's load vector and mass matrix, so the bound asserted is the one
    that follows from them: |X_1 - X_2| <= (|r_1| + |r_2|) 2 / min m (the lumped mass bounds M^-1 as in the consistent
    projection's own test)."""
    from fedm_amd import quadrature
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=6, ny=6, T_final=1.0)
    try:
        case.step()                 # (the initial potential is 0: the second step's refresh sees a field)
        case.step()
        prob = case.prob
        X2 = prob.get_gd_reduced_field()
        res = prob.gd_fields(["reduced_field"], projection="consistent", rtol=RTOL, **OLD)
        X1 = res.nodal[0]
        r = gfr.Restatement(prob.model.to_c(), case.mesh.coords, case.mesh.cells, prob.get_gd_fields(), quadrature.triangle(4))
        p = r.reference(prob.get_state_old(), "reduced_field")
        M = r.mass_matrix()
        r1, r2 = np.linalg.norm(p.b - M @ X1), np.linalg.norm(p.b - M @ X2)
        dist, bnorm = np.linalg.norm(X1 - X2), np.linalg.norm(p.b)
        allowed = (r1 + r2) * 2.0 / p.m.min()
        print(f"[gd fields] reduced field: |r_1| / |b| {r1 / bnorm:.2e} (this call, rtol {RTOL:g}), |r_2| / |b| {r2 / bnorm:.2e} "
              f"(the refresh), |X_1 - X_2| / |X| {dist / np.linalg.norm(X2):.2e}, / bound {dist / allowed:.2e}", flush=True)
        assert res.finite and res.cg_iterations[0] > 0
        assert r1 <= 2 * RTOL * bnorm
        assert dist <= allowed
    finally:
        case.prob.close()


# ---- 5: reproducible; nothing is touched ---------------------------------------------------------------------------------
def test_two_calls_agree_and_nothing_is_touched(cases):
    c = cases("two-ions-full", "irregular")
    prob = c.prob
    before = (prob.get_state(), prob.get_state_old(), prob.get_gd_fields(), prob.residual()[0])
    sets = _chunks(projected_names(c.c.md) + _pointwise_names(c.c.md))
    first = [_bytes(prob.gd_fields(n)) for n in sets]
    assert [_bytes(prob.gd_fields(n)) for n in sets] == first
    assert _bytes(prob.gd_fields(BLENDABLE, t_out=0.3, t_old=0.0, t=1.0)) == _bytes(prob.gd_fields(BLENDABLE, t_out=0.3, t_old=0.0, t=1.0))
    after = (prob.get_state(), prob.get_state_old(), prob.get_gd_fields(), prob.residual()[0])
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


# ---- 6: the blend ------------------------------------------------------------------------------------------------------
def test_blend(cases):
    c = cases("two-ions-small", "10x10")
    names = BLENDABLE
    a, b = c.prob.gd_fields(names, **OLD), c.prob.gd_fields(names)
    _check("two-ions-small 10x10 state old", a, names, lambda n: c.ref("old", n), c.c.Uo)
    assert _bytes(c.prob.gd_fields(names, t_out=2.5, t_old=1.0, t=2.5)) == _bytes(b)          # num == den
    assert _bytes(c.prob.gd_fields(names, t_out=1.0, t_old=1.0, t=2.5)) == _bytes(a)          # num == 0
    num, den = 0.3, 1.0
    mid = c.prob.gd_fields(names, t_out=num, t_old=0.0, t=den)
    expect = a.nodal + num * (b.nodal - a.nodal) / den
    err, scale = np.abs(mid.nodal - expect), np.abs(a.nodal) + np.abs(b.nodal)
    print(f"[gd fields] blend 0.3: worst error / (2 eps (|a| + |b|)) {_ratio(err, scale) / (2 * EPS):.2e}", flush=True)
    assert mid.finite and np.all(err <= 2 * EPS * scale)
    assert not np.array_equal(mid.nodal, a.nodal) and not np.array_equal(mid.nodal, b.nodal)
    # the residual's kinds and the table belong to the current step: no blend, and the next good call is what it was
    from fedm_amd.field_output import GD_KINDS as K
    for req in ("rate:0", "source:1", "collision_loss", "joule", "flux_r:0", "flux_z:1", "current_r", "current_z", "table:2"):
        with pytest.raises(RuntimeError, match=rf"request 1: {req.split(':')[0].upper()} .*num == den"):
            c.prob.gd_fields(["E_norm", req], t_out=num, t_old=0.0, t=den)
        rc, msg = _raw(c.prob, [(K["e_norm"], 0), (K[req.split(":")[0]], int(req.partition(":")[2] or 0))], num=0.0)
        assert rc == -2 and "request 1" in msg, (req, rc, msg)
    assert _bytes(c.prob.gd_fields(names)) == _bytes(b)


# ---- 7: probes ---------------------------------------------------------------------------------------------------------
def test_probes(cases):
    c = cases("deck-shape-permuted", "irregular")
    g = c.c.mesh
    rng = np.random.default_rng(17)
    x = g.coords[g.cells]
    verts = g.coords[rng.choice(g.nv, 8, replace=False)]
    ce = rng.choice(g.nc, 8, replace=False)
    s = rng.uniform(0.1, 0.9, 8)[:, None]
    edges = x[ce, 0] * s + x[ce, 1] * (1.0 - s)
    inner = np.einsum("pa,pad->pd", rng.dirichlet(np.ones(3), 8), x[rng.choice(g.nc, 8, replace=False)])
    shared = 0.5 * (g.coords[g.cells[5, 0]] + g.coords[g.cells[5, 1]])[None]       # the midpoint of an edge of cell 5
    pts = np.concatenate([verts, edges, inner, shared])
    cell, w = c.prob.gd_probe_setup(pts)
    try:
        # a point on an edge belongs to two cells: the lowest takes it
        e5 = set(g.cells[5, :2].tolist())
        sharing = [k for k in range(g.nc) if e5 <= set(g.cells[k].tolist())]
        assert cell[-1] == min(sharing) and cell[-1] <= 5
        names = ["mean_energy", "E_z", "density:3", "joule", "flux_z:0", "current_z", "source:3", "table:1"]
        both = c.prob.gd_fields(names, probes=True)
        X = both.nodal[:, g.cells[cell]]                                          # [request][point][corner]
        expect, scale = (w[None] * X).sum(axis=2), np.abs(w[None] * X).sum(axis=2)
        err = np.abs(both.probes - expect)
        print(f"[gd fields] probes: worst error / (4 eps sum|w X|) {_ratio(err, scale) / (4 * EPS):.2e}", flush=True)
        assert np.all(err <= 4 * EPS * scale)
        only = c.prob.gd_fields(names, probes=True, nodal=False)
        assert only.nodal is None and only.probes.tobytes() == both.probes.tobytes()
        with pytest.raises(ValueError, match="point 1 .*outside"):
            c.prob.gd_probe_setup(np.array([[2.5e-3, 1e-3], [1.0, 1.0]]))
        assert np.array_equal(c.prob.gd_fields(names, probes=True, nodal=False).probes, both.probes)   # the old points stand
    finally:
        c.prob.gd_fields_setup(consistent=True)                                     # (as the other tests found it: no points)


# ---- 8: not-finite input -------------------------------------------------------------------------------------------------
def test_a_nan_or_an_infinite_potential_is_flagged(cases):
    c = cases("ion-e", "10x10")
    names = ["E_norm", "joule", "charge", "rate:1"]
    first = c.prob.gd_fields(names)
    try:
        bad = c.c.U.copy()
        bad[c.c.mesh.nv // 2 + 5, 1] = np.nan
        c.prob.set_state(u_new=bad)
        assert c.prob.gd_fields(names).finite is False
        assert c.prob.gd_fields(["state:0"]).finite is False     # a request that never reads the NaN: the state is looked at
        assert c.prob.gd_fields(["E_norm", "charge"], **OLD).finite is True        # ... the state the call evaluates
        bad = c.c.U.copy()
        bad[3, int(c.c.md.n_species)] = np.inf
        c.prob.set_state(u_new=bad)
        assert c.prob.gd_fields(["E_norm"]).finite is False
        assert c.prob.gd_fields(["joule"]).finite is False
    finally:
        c.prob.set_state(u_new=c.c.U)
    again = c.prob.gd_fields(names)
    assert again.finite is True and _bytes(again) == _bytes(first)


# ---- 9: refusals through the C ABI -----------------------------------------------------------------------------------------
def _raw(prob, reqs, num=1.0, den=1.0, projection=0, rtol=1e-10, max_it=100, probes=False):
    """fedm_gd_fields through ctypes, past the host's own checks: (return code, message)."""
    from fedm_amd import _lib
    req = (_lib.FieldReq * max(len(reqs), 1))()
    for k, (kind, index) in enumerate(reqs):
        req[k].kind, req[k].index = kind, index
    o = _lib.FieldOpts()
    o.num, o.den, o.projection, o.max_it, o.rtol = num, den, projection, max_it, rtol
    out = np.empty((max(len(reqs), 1), prob.nv))
    pr_out = np.empty((max(len(reqs), 1), 64))
    fin = C.c_int32(7)
    rc = prob.lib.fedm_gd_fields(prob._h, C.byref(o), len(reqs), req, out.ctypes.data_as(C.POINTER(C.c_double)),
                                 pr_out.ctypes.data_as(C.POINTER(C.c_double)) if probes else None, C.byref(fin), None)
    return rc, _lib.last_error()


def test_refusals(cases):
    from fedm_amd import _lib, field_output
    from fedm_amd.cases import streamer
    c = cases("ion-e", "10x10")                                  # ns = 3, 4 equations, 3 reactions, 21 table rows
    names = ["E_norm", "joule", "charge", "rate:1"]
    good = c.prob.gd_fields(names)
    K = field_output.GD_KINDS

    def refused(match, *a, prob=c.prob, **k):
        rc, msg = _raw(prob, *a, **k)
        assert rc == -2 and match in msg, (match, rc, msg)

    refused("0 requests", [])
    refused("9 requests", [(K["charge"], 0)] * 9)
    refused("unknown kind 6", [(6, 0)])                          # an LFA kind's number
    refused("unknown kind 49", [(49, 0)])
    refused("index 4 out of range", [(K["state"], 4)])
    refused("index 3 out of range", [(K["density"], 3)])
    refused("index -1 out of range", [(K["flux_z"], -1)])
    refused("index 3 out of range", [(K["rate"], 3)])
    refused("index 0 out of range (1 to 2)", [(K["source"], 0)])
    refused("index 21 out of range", [(K["table"], 21)])
    refused("den of the blend is 0", [(K["charge"], 0)], num=0.5, den=0.0)
    refused("not finite", [(K["charge"], 0)], num=np.nan)
    refused("rtol is not finite", [(K["e_norm"], 0)], rtol=np.nan)
    refused("projection 2", [(K["e_norm"], 0)], projection=2)
    refused("rtol > 0", [(K["e_norm"], 0)], projection=1, rtol=0.0)
    c.prob.gd_fields_setup(consistent=True)                      # (drops the points an earlier test may have set)
    refused("no points", [(K["e_norm"], 0)], probes=True)
    verts, w = np.zeros((2, 3), dtype=np.int32), np.full((2, 3), 1.0 / 3.0)
    verts[1, 2] = c.prob.nv
    ip, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert c.prob.lib.fedm_gd_probe_setup(c.prob._h, 2, ip(verts), dp(w)) == -2
    assert f"vertex {c.prob.nv} of point 1 is out of range" in _lib.last_error()
    # before the set-up, and the consistent projection without a mass matrix
    fresh = _problem(c.c)
    try:
        refused("fedm_gd_fields_setup has not been called", [(K["charge"], 0)], prob=fresh)
        verts[1, 2] = 0
        assert fresh.lib.fedm_gd_probe_setup(fresh._h, 2, ip(verts), dp(w)) == -2
        assert "fedm_gd_fields_setup has not been called" in _lib.last_error()
        fresh.gd_fields_setup()
        refused("needs the mass matrix of fedm_gd_fields_setup", [(K["e_norm"], 0)], prob=fresh, projection=1)
        assert np.array_equal(fresh.gd_fields(names).nodal, good.nodal)
    finally:
        fresh.close()
    # an LFA context: the three calls, and the methods
    m = streamer.mesh(4)
    lfa = streamer.device_problem(m.coords, m.cells)
    try:
        assert lfa.lib.fedm_gd_fields_setup(lfa._h, None) == -2 and "LFA context" in _lib.last_error()
        assert lfa.lib.fedm_gd_probe_setup(lfa._h, 0, None, None) == -2 and "LFA context" in _lib.last_error()
        refused("LFA context", [(K["charge"], 0)], prob=lfa)
        with pytest.raises(RuntimeError, match="LMEA models only"):
            lfa.gd_fields(["charge"])
        lfa.set_state(*[np.zeros((m.coords.shape[0], 3))] * 3)
        assert lfa.fields(["charge"]).finite                     # ... and its own field output is what it was
    finally:
        lfa.close()
    # a context with ghosts
    ghosts = _problem(c.c, n_owned=c.c.mesh.nv - 3)
    try:
        assert ghosts.lib.fedm_gd_fields_setup(ghosts._h, None) == -2 and "ghost" in _lib.last_error()
        assert ghosts.lib.fedm_gd_probe_setup(ghosts._h, 0, None, None) == -2 and "ghost" in _lib.last_error()
        refused("ghost", [(K["charge"], 0)], prob=ghosts)
    finally:
        ghosts.close()
    # a refused call leaves a later good call unchanged, bit for bit
    assert _bytes(c.prob.gd_fields(names)) == _bytes(good)


# ---- 10: the case, the facade and the example --------------------------------------------------------------------------------
def test_case_fields_are_the_facades():
    from fedm_amd import functions as ff
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=6, ny=6, T_final=1.0, device_pipeline=False)
    try:
        case.step()
        names = ["mean_energy", "E_norm", "source:electrons", "joule", "density:Ar_plus"]
        assert case.species_names[-1] == "electrons" and "Ar_plus" in case.species_names
        z = np.linspace(0.0, case.gap, 9)
        pts = np.column_stack([0.0 * z, z])
        row = case.fields(names, probes=pts)
        direct = ff.Field_output(case.problem, names, probes=pts, species_names=case.species_names)()
        ns = case.ns
        plain = case.prob.gd_fields(["mean_energy", "E_norm", f"source:{ns - 1}", "joule",
                                     f"density:{case.species_names.index('Ar_plus')}"], probes=True)
        assert row["finite"] and set(row) == set(names) | {"probes", "finite"}
        for k, name in enumerate(names):
            assert np.array_equal(row[name], direct[name]) and np.array_equal(row[name], plain.nodal[k]), name
        assert np.array_equal(row["probes"], direct["probes"]) and np.array_equal(row["probes"], plain.probes)
        assert np.abs(row["joule"]).max() > 0.0 and np.all(row["mean_energy"] > 0.0)
        blended = case.fields(["mean_energy", "E_norm"], t_out=0.5 * case.t, t_old=0.0)
        assert np.array_equal(blended["E_norm"], case.prob.gd_fields(["E_norm"], t_out=0.5 * case.t, t_old=0.0, t=case.t).nodal[0])
        with pytest.raises(ValueError, match="joule"):
            case.fields(["joule"], t_out=0.5 * case.t, t_old=0.0)
    finally:
        case.prob.close()


def _example():
    spec = importlib.util.spec_from_file_location("gd_example_fields", ROOT / "examples" / "glow_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_rows_are_the_device_problems_and_the_log_is_unchanged(tmp_path):
    """examples/glow_discharge.py --fields / --axis-profile on an 8 x 8 mesh: every profile row is, to the last bit, what
    the device problem returned at that moment, the last row and the last field files are what it returns after the run
    (nothing has moved since), and `relative error.log` is the same bytes as that of a run without the options."""
    from fedm_amd import functions as ff, mesh_io
    mod = _example()
    seen = dict(problem=None, probes=[])

    def build(J, F, bcs):
        p = ff.Problem(J, F, bcs)
        asked = p.device.gd_fields

        def recording(requests, **kw):
            res = asked(requests, **kw)
            if kw.get("probes"):
                seen["probes"].append(res.probes.copy())
            return res
        p.device.gd_fields = recording
        seen["problem"] = p
        return p
    prof, names = tmp_path / "axis.txt", ["mean_energy", "joule", "source:electrons"]
    res = mod.main(nx=8, ny=8, T_final=1e-11, output_dir=tmp_path / "with", stop_before_device=build, fields=",".join(names),
                   axis_profile=prof)
    rows = np.loadtxt(prof)
    n, nf = mod.AXIS_POINTS, len(mod.AXIS_FIELDS)
    assert rows.shape == (1 + res["steps"], 1 + nf * n) and np.isnan(rows[0, 0]) and len(seen["probes"]) == res["steps"] >= 3
    assert np.array_equal(rows[0, 1:1 + n], np.linspace(0.0, mod.GAP, n)) and rows[-1, 0] == res["t"]
    for k, p in enumerate(seen["probes"]):
        assert np.array_equal(rows[1 + k, 1:], p.ravel()), k
    dev = seen["problem"].device
    del dev.gd_fields
    after = dev.gd_fields(mod.AXIS_FIELDS, probes=True, species_names=res["species"])
    assert np.array_equal(rows[-1, 1:], after.probes.ravel())
    # the run reaches the first output time, 1e-11, with its last step: one set of files, the fields of that moment
    values = dev.gd_fields(names, species_names=res["species"])
    for k, name in enumerate(names):
        stem = name.replace(":", "_")
        files = sorted((tmp_path / "with" / "fields" / stem).glob("*.vtu"))
        assert len(files) == 1, (name, files)
        assert np.array_equal(mesh_io.read_vtu(files[0], name), values.nodal[k]), name
    plain = tmp_path / "plain"
    mod.main(nx=8, ny=8, T_final=1e-11, output_dir=plain)
    log = (plain / "relative error.log").read_bytes()
    assert log == (tmp_path / "with" / "relative error.log").read_bytes() and len(log) > 0
    assert not (plain / "fields").exists() and not list(plain.glob("*axis*"))
