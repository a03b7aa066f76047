"""Field output on the device (csrc/fields.hip, DeviceProblem.fields) against the numpy restatement of
tests/field_output_reference.py, which tests/test_field_output_reference.py pins on closed forms.

Meshes of the streamer box: (a) 3 x 3 -- 18 cells, less than one wave; (b) 12 x 17 -- 408 cells, two workgroups, the
second partly empty, not square; (c) the graded Delaunay mesh of test_gpu_diagnostics._mesh, whose device numbering
moves most vertices and whose vertex valence varies.  No kernel of fields.hip caps its grid, so there is no fourth mesh.
States: the oracle's initial streamer state with photoionization_reference.perturbed, u_new != u_old.

Bounds.  Projected kinds, lumped: |dev - ref| m_v <= 1e-12 sum|terms|_v, test_gpu_diagnostics.py's SUM_BOUND for its
reason (a term's own error is about 45 eps from exp(u), two orders below).  Pointwise kinds: 4 eps of the sum of the
magnitudes of the value's addends (DENSITY: the value; CHARGE: e sum |Z_s| n_s -- each n_s carries exp's ulp on either
side, the sum and the product by e a rounding each: 3 eps for four species).  STATE: bitwise.  Consistent projection at
rtol 1e-10: |b - M X|_2 <= 2 rtol |b|_2 and |X - X_direct|_2 <= 2 |b - M X|_2 / min m_v (lambda_min(M) >= min m_v / 2).
Blend: 2 eps (|a| + |b|) against the device's own one-state results.  Probes: 4 eps sum |w_a X_a|.

MEASURED on the MI355X (every test prints its figures before it asserts).  Worst |dev - ref| m_v / sum|terms|_v of the
projected kinds: E_r, E_z, E_norm 1e-16 .. 4.6e-16; flux_r, flux_z 1e-16 .. 3.6e-15 (four species: the prescribed
drift); rate:0 2.4e-15 .. 3.5e-14 with closed-form coefficients, 2.5e-13 with tables on mesh (c) at the state whose
|E| quantiles are the knots (the rounding of grad(Phi), contracted on the device and not in numpy, carried through the
steep k(|E|): the figure nearest the bound), four species 8.5e-15, linear representation 1.3e-15.  Pointwise kinds:
density and charge up to 0.25 of the 4-eps bound (one ulp of exp), state bitwise.  Consistent projection: 11-12 CG steps
on mesh (a), 18-21 on (b) and (c); |b - M X| / |b| 1e-16 (a), 4.0e-11 .. 5.6e-11 (b, c); |X - X_direct| 0.04 .. 0.5 of
its bound.  Blend and probes: 0 (the device's sums are numpy's, bit for bit).  Ranks: owned values within 9.9e-15
(rate:0), ghosts 0.  Two processes: E_norm 2.8e-16, the axis profile 2.3e-5 of its bound.  The example: E_norm 1.7e-16,
the profile of E_z 5.4e-5 of its bound.  The whole file runs in about 9 s, no test above 2 s.
"""
import ctypes as C
import dataclasses
import importlib.util
import os
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import field_output_reference as fr  # noqa: E402
import photoionization_reference as pr  # noqa: E402
import rank_assembly_reference as rr  # noqa: E402
import tabulated_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps
SUM_BOUND, POINT_BOUND, RTOL = 1e-12, 4 * EPS, 1e-10
# every kind of the two-species models, in two calls of at most 8 requests
NAMES_A = ["state:2", "density:1", "charge", "E_r", "E_z", "E_norm", "rate:0", "flux_z:1"]
NAMES_B = ["state:0", "state:1", "density:0", "flux_r:1", "flux_r:0", "flux_z:0"]
OLD = dict(t_out=0.0, t_old=0.0, t=1.0)          # num = 0: X(u_old) alone


def _mesh(name):
    from test_gpu_diagnostics import _mesh as diag_mesh
    return diag_mesh(name)


def _models(mesh, kind):
    from test_gpu_diagnostics import _models as diag_models
    return diag_models(mesh, kind)


class Case:
    """One (mesh, model): the oracle model, the states, the restatement (computed once per (state, name), never
    changed) and one device problem with the mass matrix set up."""

    def __init__(self, mesh_name, kind):
        self.mesh = _mesh(mesh_name)
        self.om, dm, self.U_new, self.U_old = _models(self.mesh, kind)
        self.prob = tr.device_streamer_problem(self.mesh.coords, self.mesh.cells, dm)
        self.prob.set_state(self.U_new, self.U_old, self.U_old)
        self.prob.fields_setup(consistent=True)
        self._ref = {}

    def ref(self, which, name):
        if (which, name) not in self._ref:
            self._ref[which, name] = fr.reference(self.om, self.U_new if which == "new" else self.U_old, name)
        return self._ref[which, name]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(mesh_name, kind="closed"):
        if (mesh_name, kind) not in made:
            made[mesh_name, kind] = Case(mesh_name, kind)
        return made[mesh_name, kind]
    yield get
    for c in made.values():
        c.prob.close()


def _ratio(err, scale):
    """max err / scale, where scale > 0; where it is 0 the error must be 0 too."""
    assert np.all(err[scale == 0.0] == 0.0)
    return float((err[scale > 0.0] / scale[scale > 0.0]).max()) if (scale > 0.0).any() else 0.0


def _check(what, res, names, ref_of, sel=slice(None)):
    """Every request of one call against the restatement (``ref_of(name)``), on the vertices ``sel`` of the
    restatement matched to ``res.nodal``'s; prints the worst figure per request first."""
    assert res.finite
    worst = {}
    for k, name in enumerate(names):
        dev, ref = res.nodal[k], ref_of(name)
        if isinstance(ref, fr.Projected):
            worst[name] = _ratio(np.abs(dev - ref.b[sel] / ref.m[sel]) * ref.m[sel], ref.abs[sel]) / SUM_BOUND
        elif name.startswith("state"):
            worst[name] = 0.0 if np.array_equal(dev, ref.value[sel]) else np.inf
        else:
            worst[name] = _ratio(np.abs(dev - ref.value[sel]), ref.abs[sel]) / POINT_BOUND
    print(f"[fields] {what}: error / bound " + " ".join(f"{n} {v:.2e}" for n, v in worst.items()), flush=True)
    for name, v in worst.items():
        assert v <= 1.0, (what, name, v)
    return worst


def _bytes(res):
    parts = [res.nodal, res.probes, np.array([int(res.finite)]), res.cg_iterations]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts if p is not None)


# ---- 1: every kind against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("mesh_name,kind", [("a", "closed"), ("b", "closed"), ("c", "closed"), ("b", "planar"),
                                            ("c", "planar"), ("a", "tabulated"), ("b", "tabulated"), ("c", "tabulated")])
def test_every_kind_against_the_restatement(cases, mesh_name, kind):
    c = cases(mesh_name, kind)
    for which, times in (("new", {}), ("old", OLD)):
        for names in (NAMES_A, NAMES_B):
            res = c.prob.fields(names, **times)
            _check(f"mesh ({mesh_name}) {kind} state {which}", res, names, lambda n: c.ref(which, n))
    assert np.abs(c.ref("new", "flux_z:1").b).max() > 0.0 and np.all(c.ref("new", "flux_z:0").b == 0.0)
    assert not np.array_equal(c.prob.fields(["E_norm"]).nodal, c.prob.fields(["E_norm"], **OLD).nodal)


def test_four_species_with_drifting_ions():
    import lfa_models
    from oracle import streamer as ost
    m, prob, om, _, _ = lfa_models.four_species_problem()
    try:
        U2 = pr.perturbed(ost.initial_state(ost.build(om.mesh)), 22)
        r, z = m.coords[:, 0], m.coords[:, 1]
        rng = np.random.default_rng(31)
        bump = np.exp(-(r ** 2 + (z - 0.008) ** 2) / (2e-3) ** 2)
        U = np.column_stack([np.log(1e12 + 1e15 * bump) + rng.normal(0, 0.2, r.size), U2[:, 0],
                             np.log(1e11 + 1e14 * bump) + rng.normal(0, 0.2, r.size), U2[:, 1], U2[:, 2]])
        prob.set_state(U, U, U)
        for names in (["flux_z:0", "flux_z:1", "flux_z:2", "flux_z:3", "rate:0", "rate:1", "rate:2", "charge"],
                      ["flux_r:0", "flux_r:1", "flux_r:2", "flux_r:3", "E_norm", "E_r", "density:2", "state:4"]):
            _check("four species", prob.fields(names), names, lambda n: fr.reference(om, U, n))
        assert np.abs(fr.reference(om, U, "flux_r:2").b).max() > 0.0        # the prescribed drift
    finally:
        prob.close()


def test_linear_representation():
    from test_oracle_linear import _model, _state
    from fedm_amd.cases import streamer
    mesh = _mesh("b")
    om = _model(mesh, log=False)
    lnn, phi = _state(mesh, seed=9)
    U = np.column_stack([np.exp(lnn), phi])
    dm = dataclasses.replace(streamer.model(), log_representation=False)
    prob = tr.device_streamer_problem(mesh.coords, mesh.cells, dm)
    try:
        prob.set_state(U, U, U)
        for names in (NAMES_A, NAMES_B):
            _check("linear representation", prob.fields(names), names, lambda n: fr.reference(om, U, n))
        assert np.array_equal(prob.fields(["density:1"]).nodal[0], U[:, 1])
    finally:
        prob.close()


# ---- 2: the consistent projection --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh_name", ["a", "b", "c"])
def test_consistent_projection(cases, mesh_name):
    import scipy.sparse.linalg as spla
    c = cases(mesh_name)
    names = ["E_norm", "E_z", "rate:0", "flux_z:1", "charge"]
    res = c.prob.fields(names, projection="consistent", rtol=RTOL)
    assert res.finite
    M = fr.mass_matrix(c.om)
    lu = spla.splu(M.tocsc())
    print(f"[fields] mesh ({mesh_name}) consistent: CG iterations {res.cg_iterations.tolist()}", flush=True)
    assert np.all(res.cg_iterations[:4] > 0) and res.cg_iterations[4] == 0
    for k, name in enumerate(names[:4]):
        ref = c.ref("new", name)
        X = res.nodal[k]
        resid = np.linalg.norm(ref.b - M @ X)
        bnorm = np.linalg.norm(ref.b)
        dist = np.linalg.norm(X - lu.solve(ref.b))
        print(f"[fields] mesh ({mesh_name}) consistent {name}: |b - M X| / |b| {resid / bnorm:.2e}, "
              f"|X - X_direct| / (2 |b - M X| / min m) {dist * ref.m.min() / (2 * resid):.2e}", flush=True)
        assert resid <= 2 * RTOL * bnorm, name
        assert dist <= 2 * resid / ref.m.min(), name
    _check(f"mesh ({mesh_name}) consistent, the pointwise request", types.SimpleNamespace(finite=True, nodal=res.nodal[4:]),
           names[4:], lambda n: c.ref("new", n))
    assert _bytes(c.prob.fields(names, projection="consistent", rtol=RTOL)) == _bytes(res)


# ---- 3: the blend ----------------------------------------------------------------------------------------------------
def test_blend(cases):
    c = cases("c")
    names = NAMES_A
    a, b = c.prob.fields(names, **OLD), c.prob.fields(names)
    assert _bytes(c.prob.fields(names, t_out=2.5, t_old=1.0, t=2.5)) == _bytes(b)          # num == den
    assert _bytes(c.prob.fields(names, t_out=1.0, t_old=1.0, t=2.5)) == _bytes(a)          # num == 0
    num, den = 0.3, 1.0
    mid = c.prob.fields(names, t_out=num, t_old=0.0, t=den)
    expect = a.nodal + num * (b.nodal - a.nodal) / den
    err = np.abs(mid.nodal - expect)
    scale = np.abs(a.nodal) + np.abs(b.nodal)
    print(f"[fields] blend 0.3: worst error / (2 eps (|a| + |b|)) {_ratio(err, scale) / (2 * EPS):.2e}", flush=True)
    assert mid.finite and np.all(err <= 2 * EPS * scale)
    assert not np.array_equal(mid.nodal, a.nodal) and not np.array_equal(mid.nodal, b.nodal)
    try:
        c.prob.shift_state()
        assert _bytes(c.prob.fields(names, **OLD)) == _bytes(b)
        assert _bytes(c.prob.fields(names)) == _bytes(b)
    finally:
        c.prob.set_state(c.U_new, c.U_old, c.U_old)


# ---- 4: probes -------------------------------------------------------------------------------------------------------
def _probe_points(mesh):
    from oracle import streamer as ost
    rng = np.random.default_rng(17)
    x = mesh.coords[mesh.cells]
    some = lambda n, k: rng.choice(n, size=k, replace=n < k)
    verts = mesh.coords[some(mesh.nv, 16)]
    ce = some(mesh.nc, 16)
    s = rng.uniform(0.1, 0.9, 16)[:, None]
    edges = x[ce, 0] * s + x[ce, 1] * (1.0 - s)
    w = rng.dirichlet(np.ones(3), 16)
    inner = np.einsum("pa,pad->pd", w, x[some(mesh.nc, 16)])
    axis = np.column_stack([np.zeros(16), np.linspace(0.0, ost.BOX, 16)])
    return np.concatenate([verts, edges, inner, axis])


@pytest.mark.parametrize("mesh_name", ["a", "c"])
def test_probes(cases, mesh_name):
    c = cases(mesh_name)
    pts = _probe_points(c.mesh)
    assert pts.shape == (64, 2)
    cell, w = c.prob.probe_setup(pts)
    names = NAMES_A
    both = c.prob.fields(names, probes=True)
    X = both.nodal[:, c.mesh.cells[cell]]                                     # [request][point][corner]
    expect = (w[None] * X).sum(axis=2)
    scale = np.abs(w[None] * X).sum(axis=2)
    err = np.abs(both.probes - expect)
    print(f"[fields] mesh ({mesh_name}) probes: worst error / (4 eps sum|w X|) {_ratio(err, scale) / (4 * EPS):.2e}", flush=True)
    assert np.all(err <= 4 * EPS * scale)
    # a vertex probes its own nodal value
    at_vertex = np.nonzero((w == 1.0).any(axis=1))[0]
    assert at_vertex.size >= 16
    only = c.prob.fields(names, probes=True, nodal=False)
    assert only.nodal is None and np.array_equal(only.probes, both.probes) and only.probes.tobytes() == both.probes.tobytes()
    with pytest.raises(ValueError, match="point 1 .*outside"):
        c.prob.probe_setup(np.array([[1e-3, 1e-3], [1.0, 1.0]]))
    assert np.array_equal(c.prob.fields(names, probes=True, nodal=False).probes, both.probes)   # the old points stand


# ---- 5: reproducible, and the flag -----------------------------------------------------------------------------------
def test_two_calls_agree_byte_for_byte_and_a_nan_is_flagged(cases):
    c = cases("c")
    first = [c.prob.fields(n) for n in (NAMES_A, NAMES_B)]
    assert [_bytes(c.prob.fields(n)) for n in (NAMES_A, NAMES_B)] == [_bytes(r) for r in first]
    try:
        bad = c.U_new.copy()
        bad[c.mesh.nv // 2 + 5, 1] = np.nan
        c.prob.set_state(u_new=bad)
        assert c.prob.fields(NAMES_A).finite is False
        assert c.prob.fields(["state:0"]).finite is False       # a request that never reads the NaN: the state is looked at
        assert c.prob.fields(NAMES_A, **OLD).finite is True      # ... the state the call evaluates
        bad = c.U_new.copy()
        bad[3, 2] = np.inf
        c.prob.set_state(u_new=bad)
        assert c.prob.fields(["E_norm"]).finite is False
    finally:
        c.prob.set_state(u_new=c.U_new)
    again = c.prob.fields(NAMES_A)
    assert again.finite is True and _bytes(again) == _bytes(first[0])


# ---- 6: every rank of a partition, one context at a time ---------------------------------------------------------------
RANK_NAMES = ["E_norm", "rate:0", "flux_z:1", "charge"]


@pytest.fixture(scope="module")
def rank_setup():
    msh = rr.mesh()
    parts = rr.partitions(msh.coords, msh.cells)
    return dict(mesh=msh, parts=parts, cases={name: rr.CASES[name](msh) for name in ("streamer", "tabulated")})


@pytest.mark.parametrize("partition", ["r-cut", "z-cut", "three"])
@pytest.mark.parametrize("model", ["streamer", "tabulated"])
def test_ranks_owned_values(rank_setup, model, partition):
    from test_gpu_diagnostics import _create_rank
    msh, c = rank_setup["mesh"], rank_setup["cases"][model]
    om, U = c["om"], c["states"][0]
    refs = {n: fr.reference(om, U, n) for n in RANK_NAMES}
    one = tr.device_streamer_problem(msh.coords, msh.cells, c["model"]())
    try:
        one.set_state(U, U, U)
        whole = one.fields(RANK_NAMES)
    finally:
        one.close()
    _check(f"ranks: {model} on one GPU", whole, RANK_NAMES, lambda n: refs[n])
    for depth in (1, 8):
        for rank, lm in enumerate(rr.local_meshes(msh.coords, msh.cells, rank_setup["parts"][partition], depth)):
            prob = _create_rank(msh, lm, c["model"]())
            try:
                Ul = rr.restrict(lm, U)
                prob.set_state(Ul, Ul, Ul)
                res = prob.fields(RANK_NAMES)
                own, gids = slice(0, lm.n_owned), lm.vertex_global[:lm.n_owned]
                what = f"ranks: {model} {partition} depth {depth} rank {rank}"
                assert lm.n_owned < Ul.shape[0]
                assert np.all(res.nodal[:, lm.n_owned:] == 0.0), what                 # ghost entries
                _check(what, types.SimpleNamespace(finite=res.finite, nodal=res.nodal[:, own]), RANK_NAMES,
                       lambda n: refs[n], sel=gids)
                for k, n in enumerate(RANK_NAMES):                                  # ... and against the one-GPU call
                    r = refs[n]
                    scale = r.abs[gids] / r.m[gids] if isinstance(r, fr.Projected) else r.abs[gids]
                    bound = SUM_BOUND if isinstance(r, fr.Projected) else POINT_BOUND
                    assert np.all(np.abs(res.nodal[k, own] - whole.nodal[k, gids]) <= bound * scale), (what, n)
                with pytest.raises(RuntimeError, match="ghost"):
                    prob.fields_setup(consistent=True)
                prob.fields_setup()
                with pytest.raises(RuntimeError, match="ghost"):
                    prob.probe_setup(lm.coords[:2])
                with pytest.raises(RuntimeError, match="ghost"):
                    prob.fields(["E_norm"], projection="consistent")
            finally:
                prob.close()


# ---- 7: two processes ------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    from fedm_amd.cases import streamer, streamer_distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        run = streamer_distributed.Runner(None, rank, world, 0, grading=2.0, transport="torch", n_per_gpu=12)
        run.initialise()
        z = np.linspace(0.0, streamer.BOX, 33)
        out = run.fields(["E_norm", "density:electrons"], probes=np.column_stack([np.zeros_like(z), z]))
        q.put((rank, run.lm.vertex_global[:run.lm.n_owned], run.prob.get_state()[:run.lm.n_owned], out, run.global_n))
    finally:
        dist.destroy_process_group()


def test_runner_gathers_two_ranks():
    """streamer_distributed.Runner.fields on two processes sharing the GPU over the host-staged transport: the gathered
    E_norm and one axis profile against the restatement applied to the glued state."""
    import mp_results
    import torch.multiprocessing as mp
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from test_gpu_diagnostics import _free_port
    from fedm_amd import field_output
    from fedm_amd.cases import streamer
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = mp_results.collect(procs, q, len(procs), 300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    msh = streamer.mesh(res[0][4], 2.0)
    U = np.zeros((msh.coords.shape[0], 3))
    for _, gids, Uloc, _, _ in res:
        U[gids] = Uloc
    outs = {rank: out for rank, _, _, out, _ in res}
    assert outs[1] is None and outs[0]["finite"]
    om = ost.build(OMesh(msh.coords, msh.cells))
    names = ["E_norm", "density:electrons"]
    refs = [fr.reference(om, U, "E_norm"), fr.reference(om, U, "density:1")]
    _check("two ranks", types.SimpleNamespace(finite=True, nodal=np.stack([outs[0][n] for n in names])),
           ["E_norm", "density:1"], lambda n: refs[["E_norm", "density:1"].index(n)])
    z = np.linspace(0.0, streamer.BOX, 33)
    cell, w = field_output.locate_points(msh.coords, msh.cells, np.column_stack([np.zeros_like(z), z]))
    at = msh.cells[cell]
    Xref = refs[0].b / refs[0].m
    expect = (w * Xref[at]).sum(axis=1)
    allowed = (np.abs(w) * (SUM_BOUND * refs[0].abs / refs[0].m)[at]).sum(axis=1) + 4 * EPS * np.abs(w * Xref[at]).sum(axis=1)
    err = np.abs(outs[0]["probes"][0] - expect)
    print(f"[fields] two ranks: axis profile of E_norm, worst error / bound {(err / allowed).max():.2e}", flush=True)
    assert np.all(err <= allowed)


# ---- 8: refusals -----------------------------------------------------------------------------------------------------
def _raw(prob, reqs, num=1.0, den=1.0, projection=0, rtol=1e-10, max_it=100, probes=False):
    """fedm_fields through ctypes, past the host's own checks: (return code, message)."""
    from fedm_amd import _lib
    req = (_lib.FieldReq * max(len(reqs), 1))()
    for k, (kind, index) in enumerate(reqs):
        req[k].kind, req[k].index = kind, index
    o = _lib.FieldOpts()
    o.num, o.den, o.projection, o.max_it, o.rtol = num, den, projection, max_it, rtol
    out = np.empty((max(len(reqs), 1), prob.nv))
    pr_out = np.empty((max(len(reqs), 1), 64))
    fin = C.c_int32(7)
    rc = prob.lib.fedm_fields(prob._h, C.byref(o), len(reqs), req, out.ctypes.data_as(C.POINTER(C.c_double)),
                              pr_out.ctypes.data_as(C.POINTER(C.c_double)) if probes else None, C.byref(fin), None)
    return rc, _lib.last_error()


def test_refusals(cases):
    from fedm_amd import _lib, field_output
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.termsum import TermSum
    c = cases("b")
    good = c.prob.fields(NAMES_A)
    K = field_output.KINDS

    def refused(match, *a, prob=c.prob, **k):
        rc, msg = _raw(prob, *a, **k)
        assert rc == -2 and match in msg, (match, rc, msg)

    refused("index 3 out of range", [(K["state"], 3)])
    refused("index 2 out of range", [(K["density"], 2)])
    refused("index -1 out of range", [(K["flux_z"], -1)])
    refused("index 1 out of range", [(K["rate"], 1)])
    refused("unknown kind 9", [(9, 0)])
    refused("9 requests", [(K["charge"], 0)] * 9)
    refused("0 requests", [])
    refused("den of the blend is 0", [(K["charge"], 0)], num=0.5, den=0.0)
    refused("not finite", [(K["charge"], 0)], num=np.nan)
    refused("not finite", [(K["charge"], 0)], den=np.inf)
    refused("rtol is not finite", [(K["e_norm"], 0)], rtol=np.nan)
    refused("projection 2", [(K["e_norm"], 0)], projection=2)
    refused("rtol > 0", [(K["e_norm"], 0)], projection=1, rtol=0.0)
    # probes: before any points; a vertex out of range; a weight that is not finite
    c.prob.fields_setup(consistent=True)                       # (drops the points an earlier test may have set)
    refused("no points", [(K["e_norm"], 0)], probes=True)
    verts, w = np.zeros((2, 3), dtype=np.int32), np.full((2, 3), 1.0 / 3.0)
    verts[1, 2] = c.prob.nv
    ip, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert c.prob.lib.fedm_probe_setup(c.prob._h, 2, ip(verts), dp(w)) == -2
    assert f"vertex {c.prob.nv} of point 1 is out of range" in _lib.last_error()
    verts[1, 2], w[0, 1] = 0, np.inf
    assert c.prob.lib.fedm_probe_setup(c.prob._h, 2, ip(verts), dp(w)) == -2
    assert "weight 1 of point 0 is not finite" in _lib.last_error()
    # before the set-up, and the consistent projection without a mass matrix
    fresh = tr.device_streamer_problem(c.mesh.coords, c.mesh.cells, _models(c.mesh, "closed")[1])
    try:
        fresh.set_state(c.U_new, c.U_old, c.U_old)
        refused("fedm_fields_setup has not been called", [(K["charge"], 0)], prob=fresh)
        assert fresh.lib.fedm_probe_setup(fresh._h, 2, ip(verts), dp(np.full((2, 3), 1.0 / 3.0))) == -2
        assert "fedm_fields_setup has not been called" in _lib.last_error()
        fresh.fields_setup()
        refused("needs the mass matrix", [(K["e_norm"], 0)], prob=fresh, projection=1)
        assert np.array_equal(fresh.fields(NAMES_A).nodal, good.nodal)
    finally:
        fresh.close()
    # a model without a Poisson equation: E is refused, so is the flux of a drifting species without drift_w; a
    # prescribed drift and a diffusing species have their fluxes, as in fedm_diagnostics
    k = [(3.0e7, 0.5, -2.0, 1.0)]
    dm = Model(n_species=2, poisson=False, eq_type=["drift-diffusion-reaction", "drift-diffusion-reaction"], Z=[-1.0, 1.0],
               mu=[TermSum.const(0.03), TermSum.const(2e-4)], D=[TermSum.const(0.1), TermSum.const(0.2)],
               drift_w=[None, (1.0e3, -2.0e3)],
               reactions=[Reaction(TermSum(k), power=[1, 0], net=[1, 1])], bc_kind=[["zero flux"] * 2] * 4, quadrature_degree=2)
    from fedm_amd.cases import streamer
    from fedm_amd.mesh import Marking_boundaries, Mesh
    msh = Mesh(c.mesh.coords, c.mesh.cells)
    nop = DeviceProblem(msh.coords, msh.cells, dm, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES))
    try:
        U = c.U_new[:, :2]
        nop.set_state(U, U, U)
        nop.fields_setup()
        for kind in ("e_r", "e_z", "e_norm"):
            refused("needs a Poisson equation", [(K[kind], 0)], prob=nop)
        refused("drift of species 0 needs E", [(K["flux_z"], 0)], prob=nop)
        res = nop.fields(["flux_z:1", "flux_r:1", "rate:0", "charge"])
        assert res.finite and np.abs(res.nodal[0]).max() > 0.0
    finally:
        nop.close()
    # a refused call leaves a later good call unchanged, bit for bit
    assert _bytes(c.prob.fields(NAMES_A)) == _bytes(good)


def test_an_lmea_context_is_refused():
    from fedm_amd import _lib
    from fedm_amd.cases import glow_discharge as gdc
    prob = gdc.Case(device_pipeline=False, T_final=1.0, nx=3, ny=3).prob
    try:
        assert prob.lib.fedm_fields_setup(prob._h, None) == -2
        assert "LMEA" in _lib.last_error()
        rc, msg = _raw(prob, [(2, 0)])
        assert rc == -2 and "LMEA" in msg
        with pytest.raises(RuntimeError, match="LFA models only"):
            prob.fields(["charge"])
    finally:
        prob.close()


# ---- 9: the facade and the example -----------------------------------------------------------------------------------
def test_facade(cases):
    from fedm_amd import functions as ff
    c = cases("b")
    names = ["E_norm", "charge", "density:electrons", "rate:0", "flux_z:1"]
    pts = _probe_points(c.mesh)
    out = ff.Field_output(types.SimpleNamespace(device=c.prob), names, probes=pts, species_names=("ions", "electrons"))
    got = out(0.3, 0.0, 1.0)
    direct = c.prob.fields(["E_norm", "charge", "density:1", "rate:0", "flux_z:1"], t_out=0.3, t_old=0.0, t=1.0, probes=True)
    assert got["finite"] and set(got) == set(names) | {"probes", "finite"}
    for k, name in enumerate(names):
        assert np.array_equal(got[name], direct.nodal[k]), name
    assert np.array_equal(got["probes"], direct.probes)
    assert np.array_equal(out()["E_norm"], c.prob.fields(["E_norm"]).nodal[0])
    # the case's stepper: the same call with its own time as t
    from fedm_amd.cases import streamer
    st = streamer.Stepper(c.prob)
    st.t = 1.0
    row = st.fields(["E_norm", "density:electrons"], t_out=0.3, t_old=0.0, probes=pts)
    assert np.array_equal(row["E_norm"], got["E_norm"]) and np.array_equal(row["density:electrons"], got["density:electrons"])
    assert np.array_equal(row["probes"][0], got["probes"][0])
    assert np.array_equal(st.fields(["E_norm", "density:electrons"], probes=pts)["E_norm"], out()["E_norm"])
    c.prob.fields_setup(consistent=True)                                    # (as the other tests of the module found it)


def test_example_writes_fields_and_an_axis_profile(tmp_path):
    import subprocess
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from fedm_amd import field_output, mesh_io
    prof = tmp_path / "axis.txt"
    script = ROOT / "examples" / "streamer_discharge.py"
    run = subprocess.run([sys.executable, str(script), "--cells", "12", "--end", "1e-11", "--out", str(tmp_path / "out"),
                          "--fields", "E_norm,charge", "--axis-profile", str(prof), "--save-state",
                          str(tmp_path / "state.npy")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("ex_streamer_fields", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = np.loadtxt(prof)
    n = mod.AXIS_POINTS
    assert rows.shape == (3, 1 + 2 * n) and np.isnan(rows[0, 0])
    z = rows[0, 1:1 + n]
    assert np.array_equal(z, rows[0, 1 + n:]) and z[0] == 0.0 and z[-1] == mod.Case().side
    # the second step ends at the first output time exactly (2 x 5e-12 is 1e-11 in binary too): the fields written
    # there are those of the new state alone, the final state
    assert rows[1, 0] == 5e-12 and rows[2, 0] == 1e-11
    # read back through the project's reader (the VTU files hold repr(float): what was written, bit for bit)
    e_file = tmp_path / "out" / "fields" / "E_norm" / "E_norm000000.vtu"
    q_file = tmp_path / "out" / "fields" / "charge" / "charge000000.vtu"
    E, Q = mesh_io.read_vtu(e_file, "E_norm"), mesh_io.read_vtu(q_file, "charge")
    assert not (tmp_path / "out" / "fields" / "E_norm" / "E_norm000001.vtu").exists()
    U = np.load(tmp_path / "state.npy")
    mesh = mod.load_mesh(mod.Case(), 12, None, None, tmp_path)
    om = ost.build(OMesh(mesh.coords, mesh.cells))
    refE, refQ = fr.reference(om, U, "E_norm"), fr.reference(om, U, "charge")
    _check("example", types.SimpleNamespace(finite=True, nodal=np.stack([E, Q])), ["E_norm", "charge"],
           lambda nme: refE if nme == "E_norm" else refQ)
    # the profile's last row against the restatement at the final state
    cell, w = field_output.locate_points(mesh.coords, mesh.cells, np.column_stack([np.zeros(n), z]))
    at = mesh.cells[cell]
    rz = fr.reference(om, U, "E_z")
    Xz, ne = rz.b / rz.m, np.exp(U[:, 1])
    for what, got, X, tol in (("E_z", rows[2, 1:1 + n], Xz, SUM_BOUND * rz.abs / rz.m), ("n_e", rows[2, 1 + n:], ne, POINT_BOUND * ne)):
        expect = (w * X[at]).sum(axis=1)
        allowed = (np.abs(w) * tol[at]).sum(axis=1) + 4 * EPS * np.abs(w * X[at]).sum(axis=1)
        err = np.abs(got - expect)
        print(f"[fields] example: axis profile of {what}, worst error / bound {(err / allowed).max():.2e}", flush=True)
        assert np.all(err <= allowed), what
