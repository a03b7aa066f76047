"""The reduction and vector kernels of a Krylov step (csrc/kernels.hip, the second half of csrc/spmv.hip), one launch
wrapper at a time through ``DeviceProblem.krylov_op`` (``fedm_debug_krylov_op``: the production wrappers with the
production grids) against tests/krylov_kernels_reference.py, which tests/test_krylov_kernels_reference.py pins.

Inputs: basis vectors pairwise different, entries of magnitude in [0.5, 2] with random signs; distinct coefficients;
1e30 in every device entry behind the rows that take part in reductions (padding rows, and the ghost rows of a rank).
Contexts (the smallest at which each kernel can go wrong):
  a      3 x 3 streamer mesh: 16 vertices, 48 entries, under one wave; no hierarchy (an _fs op is refused there)
  b      12 x 17 streamer mesh: 234 vertices, 702 entries, 702 % 256 = 190; zero-plane mask 8 (the electron row does
         not depend on the ion density)
  b0     the same mesh, lfa_models.recombining_streamer_problem: zero-plane mask 0
  b2, b10  the same mesh, two-species models made here whose reactions leave the masks 2 and 10: with b and b0 the four
         families of spmv_dots_kernel's instantiations
  c      209 x 209 cells = 210 x 210 vertices, three equations: 132 300 entries > RED_BLOCKS * 256 = 131 072, the
         reductions' stride loop wraps
  five   lfa_models.four_species_problem(324): 325 x 325 vertices, five equations, 528 125 entries > 2048 * 256, the
         vector kernels' grid cap wraps.  Created in SECONDS_FIVE (below); no Jacobian is assembled on it
  rank   rank 0 of test_gpu_rank_assembly's r-cut with a halo of 3, no transport: n_owned < nv, n_dot < n

Bounds, set in advance (none is tuned to the device's result):
  sums      |device - fsum| <= 1e-12 sum |terms|    (tests/test_gpu_diagnostics.py's standing condition)
  updates   per entry (K + 2) eps (|y_i| + sum |c_k x_k,i|) |scale|   (K + 1 roundings of a chain of K products and
            sums and one of the scale, each at most eps / 2 of the running magnitude; only FMA contraction may differ)
  g32       2^-23 sum |dinv t| per entry (one rounding to single precision, 2^-24, and the float64 sum's)
  formulae  on the device's own published sums: hn2 within (k + 1) eps ww, scale within 2 ulp
  w         (width + 2) eps (|J| |z|) per row of the fused product

The plane masks: the streamer's is 8 and the recombining streamer's 0; 2 and 10 come from two models made here.

MEASURED (below) holds the worst figure per family on an MI355X; DESIGN.md section 5 has the same table.
"""
import math
import time

import numpy as np
import pytest

import krylov_kernels_reference as kk

pytestmark = pytest.mark.gpu

EPS = kk.EPS
SUM_BOUND = 1e-12
SENTINEL = 1e30
K_DOTS = (1, 2, 7, 8, 9, 16, 17, 32)
K_UPDATE = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 30)

# Measured on an MI355X, 2026-10-20, all 264 cases (each test prints its own figure before it asserts; 1 279 figures in
# all).  Per family the worst one, in the unit its bound is stated in.  No fault was found: nothing here was fixed.
MEASURED = {
    "sums": 2.92e-16,        # |dev - fsum| / sum |terms| (bound 1e-12): spmv_dots on the rank, k = 8; 616 sums
    "updates": 0.607,        # of (K + 2) eps magnitude: the update of a refined step, context c, k = 2; 321 vectors
    "g32": 0.0,              # of 2^-23 sum |dinv t|: every one of the 18 comparisons equal to the last bit of float32
    "hn2": 0.141,            # of (k + 1) eps ww: dots_fused, context a, k = 7, w in the span; 262 finishes
    "scale_ulp": 0.0,        # ulp (bound 2): every scale equal to 1 / sqrt(hn2) of the published hn2
    "product": 0.085,        # of (width + 2) eps |J| |z|: context c, k = 8; 147 products
}
# Creation of the 325 x 325 five-equation context (105 625 vertices), measured: 0.2 s; no Jacobian is assembled on it.
# The contexts of test_gpu_fullsize.py have three to twelve times as many vertices (577 x 577 and 1153 x 1153), so the
# mesh stays at 325 x 325.  The whole file: 19 s, the slowest case 2.5 s (the first one of the five-equation context,
# which computes its shared sums).
SECONDS_FIVE = 0.2


# ---- contexts ------------------------------------------------------------------------------------------------------
class Context:
    """A device problem and the inputs every test of it shares: 32 basis vectors, y, x0, their exact sums (computed
    once, never changed)."""

    def __init__(self, name, prob, jacobian):
        self.name, self.prob = name, prob
        self.neq, self.nv, self.n = prob.n_eq, prob.nv, prob.n
        self.n_owned = prob.n_owned
        self.n_dot = self.n_owned * self.neq
        self.np_ = ((self.nv + 63) // 64) * 64 * self.neq
        seed = sum(ord(ch) for ch in name)
        rng = np.random.default_rng(seed)
        self.V = self._vectors(rng, 32)
        self.y, self.x = self._vectors(rng, 2)
        self.x0 = rng.uniform(0.5, 2.0, self.nv) * rng.choice([-1.0, 1.0], self.nv)
        self.J = prob.jacobian_csr(device_order=True) if jacobian else None
        self._dots = {}

    def _vectors(self, rng, count):
        v = rng.uniform(0.5, 2.0, (count, self.n)) * rng.choice([-1.0, 1.0], (count, self.n))
        v[:, self.n_dot:] = SENTINEL          # what the device holds there: the restatement sees the same vectors
        return v

    def pad(self, v):
        return kk.padded(v, self.n_dot, self.np_, SENTINEL)

    def exact_dots(self, key, V, y, wgt=None):
        """fsum of V[i] . y for all of V, cached under `key`."""
        if key not in self._dots:
            self._dots[key] = kk.dots(V, y, self.n_dot, len(V), wgt=wgt)
        return self._dots[key]

    def sound_y(self):
        """y with its components along the 31 basis vectors taken out (normal equations) and 1e-3 v_i / |v_i| of each
        put back: h_i of about 1e-3 |v_i|, hn2 / ww close to 1."""
        if not hasattr(self, "_sound"):
            d = self.n_dot
            A = self.V[:31, :d]
            y = self.y.copy()
            y[:d] -= A.T @ np.linalg.solve(A @ A.T, A @ y[:d])
            y[:d] += 1e-3 * (A / np.linalg.norm(A, axis=1)[:, None]).sum(axis=0)
            self._sound = y
        return self._sound

    def orthonormal(self):
        """31 orthonormal vectors over the rows that take part in reductions (QR of the basis; the first m of them span
        what the first m basis vectors span): what the finish formulae presume, sum h_i^2 <= ww."""
        if not hasattr(self, "_Q"):
            Q, _ = np.linalg.qr(self.V[:31, :self.n_dot].T)
            self._Q = np.array([self.pad(q)[:self.n] for q in Q.T])
        return self._Q

    def in_span(self, m):
        """A vector in the span of the first m orthonormal vectors."""
        Q = self.orthonormal()
        return self.pad(np.linspace(1.0, 2.0, m) @ Q[:m, :self.n_dot])[:self.n]


def _streamer_state(prob):
    from fedm_amd.cases import streamer
    U = np.zeros((prob.nv, 3))
    U[:, 0], U[:, 1] = streamer.initial_log_densities(prob.coords)
    U[:, 2] = streamer.U_W * prob.coords[:, 1] / streamer.BOX
    prob.set_state(U, U - 0.01, U - 0.02)
    prob.set_step(5e-12, 4e-12)


def _masked_problem(coords, cells, name):
    """The streamer's transport with other reactions: none (b10: neither species row depends on the other species), or
    electrons made at a rate proportional to the ion density (b2: only the ion row is independent of the electrons)."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem, Model, Reaction
    from fedm_amd.mesh import Marking_boundaries, Mesh
    from fedm_amd.termsum import TermSum, parse
    msh = Mesh(coords, cells)
    reactions = [] if name == "b10" else [Reaction(TermSum.const(1e3), power=[1, 0], net=[0, 1])]
    model = Model(n_species=2, poisson=True, eq_type=["reaction", "drift-diffusion-reaction"], Z=[1.0, -1.0],
                  mu=[TermSum.const(0.0), parse(streamer.MU_E)], D=[TermSum.const(0.0), parse(streamer.D_E)],
                  reactions=reactions, bc_kind=streamer.BC_TYPE, quadrature_degree=2)
    dofs, vals = streamer.dirichlet(msh.coords)
    return DeviceProblem(msh.coords, msh.cells, model, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                         dirichlet_dofs=dofs, dirichlet_vals=vals)


def _make(name):
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    if name == "five":
        from lfa_models import four_species_problem
        t0 = time.time()
        prob = four_species_problem(324, 2.0, oracle_model=False)[1]
        print(f"[krylov kernels] context five: {prob.nv} vertices, {prob.n} entries, created in "
              f"{time.time() - t0:.1f} s", flush=True)
        assert prob.n == 325 * 325 * 5 > kk.VEC_BLOCKS * 256
        return Context(name, prob, False)
    if name == "rank":
        import rank_assembly_reference as rr
        from test_gpu_rank_assembly import _create
        msh = rr.mesh()
        lm = rr.local_meshes(msh.coords, msh.cells, rr.partitions(msh.coords, msh.cells)["r-cut"], 3)[0]
        prob = _create(msh, lm, streamer.model())
        assert prob.n_owned < prob.nv
    else:
        from oracle import streamer as ost
        from oracle.mesh import rectangle_right
        nx, ny = {"a": (3, 3), "c": (209, 209)}.get(name, (12, 17))
        m = rectangle_right(0.0, 0.0, ost.BOX, ost.BOX, nx, ny)
        if name == "b0":
            from lfa_models import recombining_streamer_problem
            prob = recombining_streamer_problem(m.coords, m.cells)
        elif name in ("b2", "b10"):
            prob = _masked_problem(m.coords, m.cells, name)
        else:
            prob = streamer.device_problem(m.coords, m.cells)
    _streamer_state(prob)
    if name in ("b", "c"):
        prob.setup_multigrid(nu=1, omega=0.85, max_coarse=40 if prob.nv < 5000 else 2000)
        prob.set_fieldsplit(chebyshev_weights(6))
    prob.jacobian()
    ctx = Context(name, prob, True)
    if name == "b":
        assert ctx.n_dot % 256 not in (0, 1)
    if name == "c":
        assert ctx.n_dot == 132300 > kk.RED_BLOCKS * 256
    return ctx


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make(name)
        return made[name]
    yield get
    for c in made.values():
        c.prob.close()


ALL = ("a", "b", "c", "five", "rank")


# ---- checks ----------------------------------------------------------------------------------------------------------
def _check_sums(label, got, ref, mag):
    got, ref, mag = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got, ref, mag))
    if got.size == 0:
        return 0.0
    fig = float(np.max(np.abs(got - ref) / mag))
    print(f"[krylov kernels] {label}: sums worst |dev - fsum| / sum|terms| = {fig:.2e} (bound {SUM_BOUND:.0e})", flush=True)
    assert np.isfinite(got).all()
    assert fig <= SUM_BOUND, (label, fig)
    return fig


def _check_update(label, got, ref, mag, K):
    bound = (K + 2) * EPS * mag
    fig = float(np.max(np.abs(got - ref) / bound))
    print(f"[krylov kernels] {label}: update worst |dev - ref| / bound = {fig:.3f}", flush=True)
    assert np.isfinite(got).all()
    assert fig <= 1.0, (label, fig)
    return fig


def _ulps(a, b):
    return abs(a - b) / np.spacing(abs(b))


def _check_formulae(label, row, k, orthonormal=True):
    """The finish formulae on the device's own sums: row = a finished reduction row.  hn2 within (k + 1) eps ww: k
    roundings of the sum of squares and one of the difference, with sum h_i^2 <= ww as an orthonormal basis gives it
    (Bessel).  orthonormal=False, inputs outside that premise (sum h_i^2 may be many times ww): the same roundings
    relative to ww + sum h_i^2, and no statement about which side of the test the input is on."""
    h, ww, hn2, scale = row[:k - 1], row[kk.RED_K - 2], row[k - 1], row[kk.RED_K - 1]
    hn2_ref, _, _ = kk.finish_values(h, ww)
    if not orthonormal:
        assert abs(hn2 - hn2_ref) <= (k + 1) * EPS * (abs(ww) + float(np.sum(h * h))), label
        expect_scale = (1.0 / math.sqrt(hn2)) if (hn2 > 1e-8 * ww and hn2 > 0.0) else 1.0
        assert _ulps(scale, expect_scale) <= 2.0, label
        return hn2 > 1e-8 * ww and hn2 > 0.0
    scale_of_dev = (1.0 / math.sqrt(hn2)) if (hn2 > 1e-8 * ww and hn2 > 0.0) else 1.0
    ratio = hn2 / ww if ww > 0.0 else float("-inf")          # (ww <= 0 only where slot k - 1 is no squared norm)
    print(f"[krylov kernels] {label}: hn2 {hn2:.6e} ww {ww:.6e} |hn2 - ref| / ((k+1) eps ww) = "
          f"{abs(hn2 - hn2_ref) / ((k + 1) * EPS * abs(ww)):.3f}, scale {scale:.6e} off by "
          f"{_ulps(scale, scale_of_dev):.1f} ulp, hn2/ww {ratio:.3e}", flush=True)
    assert abs(hn2 - hn2_ref) <= (k + 1) * EPS * abs(ww), label
    assert ratio >= 1e-3 or ratio <= 1e-12, (label, "an input that is neither sound nor unsound by a margin")
    assert _ulps(scale, scale_of_dev) <= 2.0, label
    return ratio >= 1e-3


def _check_counts(out, published):
    assert out["published"] == published and out["host_seq"] == out["device_seq"]
    assert (out["mail"] is not None) == (published > 0)


def _pattern():
    """Distinct contents for both reduction rows: what an op must carry through shows."""
    return np.arange(1.0, 2 * kk.RED_K + 1.0).reshape(2, kk.RED_K) * 0.125


# ---- launch_dots -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", K_DOTS)
@pytest.mark.parametrize("name", ALL)
def test_dots(contexts, name, k):
    c = contexts(name)
    ref, mag = c.exact_dots("V.y", c.V, c.y)
    out = c.prob.krylov_op("dots", k, V=c.V[:k], y=c.y, red=_pattern())
    _check_counts(out, 0)
    _check_sums(f"dots {name} k={k}", out["red"][0, :k], ref[:k], mag[:k])
    assert np.array_equal(out["red"][0, k:], _pattern()[0, k:]) and np.array_equal(out["red"][1], _pattern()[1])
    # with the finish: cgs_finish_kernel works in place.  The random basis is not orthonormal (sum h^2 >> ww) ...
    Vk = np.vstack([c.V[:k - 1], c.y[None, :]])
    out = c.prob.krylov_op("dots", k, V=Vk, y=c.y, red=_pattern(), finish=1)
    _check_counts(out, 1)
    assert np.array_equal(out["mail"], out["red"][0])
    assert np.array_equal(out["red"][0, k:kk.RED_K - 2], _pattern()[0, k:kk.RED_K - 2])
    if k > 1 and not _check_formulae(f"dots+finish {name} k={k} random", out["red"][0], k, orthonormal=False):
        assert out["red"][0, kk.RED_K - 1] == 1.0
    # ... an orthonormal one with a sound w (its components along the basis small) ...
    Q, ys = c.orthonormal(), c.sound_y()
    Vk = np.vstack([Q[:k - 1], ys[None, :]])
    out = c.prob.krylov_op("dots", k, V=Vk, y=ys, finish=1)
    _check_counts(out, 1)
    refs, mags = c.exact_dots("Q.ys", np.vstack([Q, ys[None, :]]), ys)
    _check_sums(f"dots+finish {name} k={k} h", out["red"][0, :k - 1], refs[:k - 1], mags[:k - 1])
    _check_sums(f"dots+finish {name} k={k} ww", out["red"][0, kk.RED_K - 2], refs[31], mags[31])
    assert _check_formulae(f"dots+finish {name} k={k} sound", out["red"][0], k)
    expect = kk.finish(np.append(out["red"][0, :k - 1], out["red"][0, kk.RED_K - 2]), k, np.zeros(kk.RED_K), "cgs")
    assert np.array_equal(np.delete(out["red"][0], [k - 1, kk.RED_K - 1]), np.delete(expect, [k - 1, kk.RED_K - 1]))
    # ... and with w in its span: hn2 <= 0 up to rounding, scale 1
    if k > 1:
        yin = c.in_span(k - 1)
        out = c.prob.krylov_op("dots", k, V=np.vstack([Q[:k - 1], yin[None, :]]), y=yin, finish=1)
        assert not _check_formulae(f"dots+finish {name} k={k} span", out["red"][0], k)
        assert out["red"][0, kk.RED_K - 1] == 1.0


# ---- launch_dots_fused -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", K_DOTS)
@pytest.mark.parametrize("name", ALL)
def test_dots_fused(contexts, name, k):
    c = contexts(name)
    ref, mag = c.exact_dots("V.y", c.V, c.y)
    # y a vector of its own, no x0, no finish: the plain sums through dots_scatter_kernel
    out = c.prob.krylov_op("dots_fused", k, V=c.V[:k], y=c.y, red=_pattern())
    _check_counts(out, 0)
    _check_sums(f"dots_fused {name} k={k} plain", out["red"][0, :k], ref[:k], mag[:k])
    assert np.array_equal(out["y"], c.y) and np.array_equal(out["red"][0, k:], _pattern()[0, k:])
    # y among the basis (the last slot: ww), x0 scattered into it, finish: reduce_finish_kernel
    for y_index in sorted({k - 1, 0}):
        s_ref, s_mag, y_ref = kk.dots_fused(c.V[:k], None, c.n_dot, k, c.neq, x0=c.x0, y_index=y_index)
        out = c.prob.krylov_op("dots_fused", k, V=c.V[:k], x0=c.x0, y_index=y_index, red=_pattern(), finish=1)
        _check_counts(out, 1)
        assert np.array_equal(out["y"], y_ref), (name, k, y_index)          # the scatter is a copy: exact
        row = out["red"][0]
        sums = np.append(row[:k - 1], row[kk.RED_K - 2])
        _check_sums(f"dots_fused {name} k={k} y=V[{y_index}] x0", sums, s_ref, s_mag)
        assert np.array_equal(out["mail"], row)
        expect = kk.finish(sums, k, _pattern()[0], "reduce")                 # the rest 0, RED_SPARE carried through
        assert np.array_equal(np.delete(row, [k - 1, kk.RED_K - 1]), np.delete(expect, [k - 1, kk.RED_K - 1]))
        if k > 1:
            _check_formulae(f"dots_fused {name} k={k} y=V[{y_index}]", row, k, orthonormal=False)
    # y of its own with x0, no finish
    s_ref, s_mag, y_ref = kk.dots_fused(c.V[:k], c.y, c.n_dot, k, c.neq, x0=c.x0)
    out = c.prob.krylov_op("dots_fused", k, V=c.V[:k], y=c.y, x0=c.x0)
    assert np.array_equal(out["y"], y_ref)
    _check_sums(f"dots_fused {name} k={k} own y, x0", out["red"][0, :k], s_ref, s_mag)
    # an orthonormal basis: a sound w, and w in the span
    Q, ys = c.orthonormal(), c.sound_y()
    refs, mags = c.exact_dots("Q.ys", np.vstack([Q, ys[None, :]]), ys)
    Vk = np.vstack([Q[:k - 1], ys[None, :]])
    out = c.prob.krylov_op("dots_fused", k, V=Vk, y_index=k - 1, finish=1)
    _check_sums(f"dots_fused {name} k={k} sound h", out["red"][0, :k - 1], refs[:k - 1], mags[:k - 1])
    assert _check_formulae(f"dots_fused {name} k={k} sound", out["red"][0], k)
    if k > 1:
        out = c.prob.krylov_op("dots_fused", k, V=np.vstack([Q[:k - 1], c.in_span(k - 1)[None, :]]), y_index=k - 1, finish=1)
        assert not _check_formulae(f"dots_fused {name} k={k} span", out["red"][0], k)
        assert out["red"][0, kk.RED_K - 1] == 1.0


def test_finish_with_w_in_the_span_of_the_basis(contexts):
    """hn2 <= 0 (or far below 1e-8 ww): scale 1, for the host to refine."""
    c = contexts("b")
    d = c.n_dot
    Q, _ = np.linalg.qr(c.V[:4, :d].T)
    V = np.array([c.pad(q)[:c.n] for q in Q.T])
    w = c.pad(Q @ np.array([1.0, -2.0, 0.5, 3.0]))[:c.n]
    for op, extra in (("dots", dict(y=w)), ("dots_fused", dict(y_index=4))):
        out = c.prob.krylov_op(op, 5, V=np.vstack([V, w[None, :]]), finish=1, **extra)
        row = out["red"][0]
        print(f"[krylov kernels] span {op}: hn2 {row[4]:.3e} ww {row[kk.RED_K - 2]:.3e}", flush=True)
        assert row[4] <= 1e-12 * row[kk.RED_K - 2] and row[kk.RED_K - 1] == 1.0
        assert abs(row[4]) <= 6 * EPS * row[kk.RED_K - 2]


# ---- launch_spmv_dots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2, 9))
@pytest.mark.parametrize("name", ("a", "b", "b0", "b2", "b10", "c", "rank"))
def test_spmv_dots(contexts, name, k):
    c = contexts(name)
    mask = c.prob.plane_masks()[1]
    if name.startswith("b"):
        assert mask == {"b": 8, "b0": 0, "b2": 2, "b10": 10}[name]
    z = c.x.copy()
    z[c.n_dot:] = c.V[0, :c.n - c.n_dot] if c.n > c.n_dot else 0.0      # ghost entries are operands: ordinary values
    w_ref, w_mag, s_ref, s_mag = kk.spmv_dots(c.J, z, c.V, c.n_owned, c.neq, k)
    width = int(np.diff(c.J.indptr).max())
    for finish in (0, 1, 2):
        out = c.prob.krylov_op("spmv_dots", k, V=c.V[:k - 1], x=z, red=_pattern(), finish=finish)
        _check_counts(out, 1 if finish == 1 else 0)
        w = out["y"]
        bound = (width + 2) * EPS * w_mag
        rows = w_mag > 0
        fig = float(np.max(np.abs(w - w_ref)[rows] / bound[rows]))
        print(f"[krylov kernels] spmv_dots {name} mask {mask} k={k} finish={finish}: product worst / bound {fig:.3f}", flush=True)
        assert fig <= 1.0 and np.all(w[~rows] == 0.0)
        assert np.all(w[c.n_dot:] == 0.0)                                  # ghost rows written as 0
        row = out["red"][0]
        if finish == 0:
            _check_sums(f"spmv_dots {name} k={k} sums", row[:k], s_ref, s_mag)
            assert np.array_equal(row[k:], _pattern()[0, k:])
            continue
        sums = np.append(row[:k - 1], row[kk.RED_K - 2])
        _check_sums(f"spmv_dots {name} k={k} finish={finish}", sums, s_ref, s_mag)
        sound = _check_formulae(f"spmv_dots {name} k={k} finish={finish}", row, k, orthonormal=False)
        expect = kk.finish(sums, k, _pattern()[0], "reduce", flag_refine=finish == 2)
        expect[kk.RED_REFINE] = (0.0 if sound else 1.0) if finish == 2 else 0.0
        assert np.array_equal(np.delete(row, [k - 1, kk.RED_K - 1]), np.delete(expect, [k - 1, kk.RED_K - 1]))
        if finish == 1:
            assert np.array_equal(out["mail"], row)
        assert np.array_equal(out["red"][1], _pattern()[1])
    # an orthonormal basis, as the formulae presume: w = J z has most of itself outside a few random directions (sound,
    # flag 0); with w / |w| as the one basis vector it lies in the span (flag 1, scale 1)
    Q = c.orthonormal()
    for finish in (1, 2):
        row = c.prob.krylov_op("spmv_dots", k, V=Q[:k - 1], x=z, finish=finish)["red"][0]
        assert _check_formulae(f"spmv_dots {name} k={k} finish={finish} orthonormal", row, k)
        assert row[kk.RED_REFINE] == 0.0
    if k == 2:
        unit = w_ref / np.linalg.norm(w_ref)
        unit[c.n_dot:] = SENTINEL
        for finish in (1, 2):
            row = c.prob.krylov_op("spmv_dots", 2, V=unit[None, :], x=z, finish=finish)["red"][0]
            assert not _check_formulae(f"spmv_dots {name} finish={finish} span", row, 2)
            assert row[kk.RED_K - 1] == 1.0 and row[kk.RED_REFINE] == (1.0 if finish == 2 else 0.0)


# ---- launch_cgs_refine -----------------------------------------------------------------------------------------------
def _orthonormal(c, count):
    Q, _ = np.linalg.qr(c.V[:count, :c.n_dot].T)
    return np.array([c.pad(q)[:c.n] for q in Q.T]), Q


def _first_stage_check(label, c, out, t_dev):
    dinv = kk.species_block_inverses(c.J, c.nv, 2)
    g, mag, b0 = kk.first_stage(t_dev, dinv, c.nv, 2)
    fig = float(np.max(np.abs(out["g32"].astype(np.float64) - g) / (2.0 ** -23 * mag)))
    print(f"[krylov kernels] {label}: g32 worst |dev - ref| / (2^-23 sum|dinv t|) = {fig:.3f}", flush=True)
    assert np.isfinite(out["g32"]).all() and fig <= 1.0
    assert np.array_equal(out["b0"], b0)


@pytest.mark.parametrize("k", (2, 3, 4, 5))
@pytest.mark.parametrize("name", ("b", "c"))
def test_cgs_refine(contexts, name, k):
    c = contexts(name)
    V, Q = _orthonormal(c, k - 1)
    t = c.y
    red = _pattern()
    red[0, kk.RED_REFINE] = 0.0
    # flag 0: nothing is touched, byte for byte, and the one publication carries what the first finish left
    out = c.prob.krylov_op("cgs_refine", k, V=V, y=t, red=red)
    _check_counts(out, 1)
    assert out["red"].tobytes() == red.tobytes() and out["y"].tobytes() == t.tobytes()
    assert out["mail"].tobytes() == red[0].tobytes()
    # flag 1, sound
    red[0, kk.RED_REFINE] = 1.0
    r_ref, t_ref, t_mag, s_ref, s_mag = kk.refine(red, [c.pad(v) for v in V], c.pad(t), c.n_dot, k)
    out = c.prob.krylov_op("cgs_refine", k, V=V, y=t, red=red)
    _check_counts(out, 1)
    row, coef = out["red"]
    _check_sums(f"refine {name} k={k} c", coef[:k - 1], s_ref[:k - 1], s_mag[:k - 1])
    tt = row[k - 1] + float(np.sum(coef[:k - 1] ** 2))                     # (tt itself is not published)
    assert abs(tt - s_ref[k - 1]) <= SUM_BOUND * s_mag[k - 1] + (k + 1) * EPS * s_ref[k - 1]
    assert row[kk.RED_REFINE] == 1.0 and row[kk.RED_SPARE] == red[0, kk.RED_SPARE]
    assert np.array_equal(row[:k - 1], red[0, :k - 1] + coef[:k - 1])
    assert row[kk.RED_K - 1] == coef[kk.RED_K - 1] and _ulps(row[kk.RED_K - 1], 1.0 / math.sqrt(row[k - 1])) <= 2.0
    assert np.array_equal(out["mail"], row)
    # the update with the device's own coefficients
    t_own, mag_own = kk.cgs_update(c.pad(t), [c.pad(v) for v in V], coef, k - 1)
    _check_update(f"refine {name} k={k} t", out["y"], t_own[:c.n], mag_own[:c.n], k - 1)
    _first_stage_check(f"refine {name} k={k}", c, out, out["y"])
    # flag 1 with t in the span of V: flag 2 and scale 1
    t_in = c.pad(Q @ np.linspace(1.0, 2.0, k - 1))[:c.n]
    out = c.prob.krylov_op("cgs_refine", k, V=V, y=t_in, red=red)
    print(f"[krylov kernels] refine {name} k={k} span: hn2' {out['red'][0, k - 1]:.3e}", flush=True)
    assert out["red"][0, kk.RED_REFINE] == 2.0 and out["red"][0, kk.RED_K - 1] == 1.0 == out["red"][1, kk.RED_K - 1]
    _check_counts(out, 1)


# ---- launch_norm2, norm2_publish ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_norm2_and_its_publication(contexts, name):
    c = contexts(name)
    ref, mag = kk.norm2(c.y, c.n_dot)
    for slot in (0, 1, kk.RED_SPARE):
        out = c.prob.krylov_op("norm2", y=c.y, slot=slot, red=_pattern())
        _check_counts(out, 0)
        _check_sums(f"norm2 {name} slot {slot}", out["red"][0, slot], ref, mag)
        assert np.array_equal(np.delete(out["red"][0], slot), np.delete(_pattern()[0], slot))
    for slot, k in ((0, 1), (0, 5), (2, 3)):
        out = c.prob.krylov_op("norm2_publish", k, y=c.y, slot=slot, red=_pattern())
        _check_counts(out, 1)
        _check_sums(f"norm2_publish {name} slot {slot} k {k}", out["red"][0, slot], ref, mag)
        assert np.array_equal(out["mail"][:k], out["red"][0, :k])
        assert np.array_equal(np.delete(out["red"][0], slot), np.delete(_pattern()[0], slot))


# ---- the updates -------------------------------------------------------------------------------------------------------
def _coefficients(k):
    return np.array([(-1.0) ** i * (0.3 + 0.07 * i) for i in range(k)])


@pytest.mark.parametrize("k", K_UPDATE)
@pytest.mark.parametrize("name", ALL)
def test_cgs_update_and_multi_axpy(contexts, name, k):
    c = contexts(name)
    red = _pattern()
    red[0, :k] = _coefficients(k)
    red[0, kk.RED_K - 1] = 0.37
    Vp, yp = [c.pad(v) for v in c.V[:k]], c.pad(c.y)
    ref, mag = kk.cgs_update(yp, Vp, red[0], k)
    out = c.prob.krylov_op("cgs_update", k, V=c.V[:k], y=c.y, red=red)
    _check_counts(out, 0)
    _check_update(f"cgs_update {name} k={k}", out["y"], ref[:c.n], mag[:c.n], k)
    assert np.array_equal(out["red"], red)
    for sign in (1.0, -1.0):
        ref, mag = kk.multi_axpy(yp, Vp, red[0, :k], k, sign=sign)
        out = c.prob.krylov_op("multi_axpy", k, V=c.V[:k], y=c.y, coef=red[0, :k], a=sign)
        _check_update(f"multi_axpy {name} k={k} sign {sign:+.0f}", out["y"], ref[:c.n], mag[:c.n], k)


@pytest.mark.parametrize("k", range(1, 9))
@pytest.mark.parametrize("name", ALL)
def test_newton_update(contexts, name, k):
    c = contexts(name)
    coef = _coefficients(k)
    Vp, up = [c.pad(v) for v in c.V[:k]], c.pad(c.y)
    un, d, mag, mag_d, (dd, md), (uu, mu) = kk.newton_update(up, Vp, coef, k, c.n_dot)
    for store in (1, 0):
        out = c.prob.krylov_op("newton_update", k, V=c.V[:k], y=c.y, coef=coef, finish=store, red=_pattern())
        _check_counts(out, 0)
        _check_update(f"newton_update {name} k={k} u", out["y"], un[:c.n], mag[:c.n], k)
        if store:
            _check_update(f"newton_update {name} k={k} delta", out["x"], d[:c.n], mag_d[:c.n], k)
        else:
            assert np.all(out["x"] == SENTINEL)                            # delta is not stored
        _check_sums(f"newton_update {name} k={k}", out["red"][0, 1:3], [dd, uu], [md, mu])
        assert np.array_equal(np.delete(out["red"][0], [1, 2]), np.delete(_pattern()[0], [1, 2]))


@pytest.mark.parametrize("k", (1, 2, 3, 4))
@pytest.mark.parametrize("name", ("b", "c"))
def test_updates_with_the_first_stage(contexts, name, k):
    c = contexts(name)
    red = _pattern()
    red[0, :k] = _coefficients(k)
    red[0, kk.RED_K - 1] = 0.37
    ref, mag = kk.cgs_update(c.pad(c.y), [c.pad(v) for v in c.V[:k]], red[0], k)
    out = c.prob.krylov_op("cgs_update_fs", k, V=c.V[:k], y=c.y, red=red)
    _check_counts(out, 0)
    _check_update(f"cgs_update_fs {name} k={k}", out["y"], ref[:c.n], mag[:c.n], k)
    _first_stage_check(f"cgs_update_fs {name} k={k}", c, out, out["y"])
    if k == 1:
        out = c.prob.krylov_op("scale_copy_fs", x=c.x, a=-0.37)
        assert np.array_equal(out["y"], -0.37 * c.x)
        _first_stage_check(f"scale_copy_fs {name}", c, out, out["y"])


@pytest.mark.parametrize("name", ALL)
def test_normalise_copy(contexts, name):
    c = contexts(name)
    red = _pattern()
    for slot, n2 in ((0, 7.3), (3, 0.0), (3, math.inf), (5, -1.0), (5, math.nan)):
        red[0, slot] = n2
        out = c.prob.krylov_op("normalise_copy", x=c.x, slot=slot, red=red)
        ref = kk.normalise_copy(c.pad(c.x), n2)[:c.n]
        if n2 == 7.3:
            _check_update(f"normalise_copy {name}", out["y"], ref, np.abs(ref), 0)
        else:
            assert not out["y"].any(), (name, n2)                          # a zero, infinite or undefined norm: y = 0


@pytest.mark.parametrize("name", ALL)
def test_field_error(contexts, name):
    c = contexts(name)
    state = c.prob.get_state().copy()
    for op, slots in (("field_error", [0, 1]), ("field_error_slots34", [3, 4])):
        for comp in range(c.neq):
            (d, md), (o, mo) = kk.field_error(c.y, c.x, c.n_owned, c.neq, comp)
            out = c.prob.krylov_op(op, y=c.y, x=c.x, slot=comp, red=_pattern())
            _check_sums(f"{op} {name} component {comp}", out["red"][0, slots], [d, o], [md, mo])
            assert np.array_equal(np.delete(out["red"][0], slots), np.delete(_pattern()[0], slots))
    assert np.array_equal(c.prob.get_state(), state)                       # the state came back


# ---- the weighted forms ------------------------------------------------------------------------------------------------
def test_weighted_reductions(contexts):
    c = contexts("b")
    c.prob.set_krylov_scaling("rows")
    try:
        d = c.prob._vec(c.prob.krylov_scaling()[1])
        wgt = c.pad(d * d)
        assert wgt[:c.n_dot].min() > 0 and wgt[:c.n_dot].max() / wgt[:c.n_dot].min() > 10.0    # weights that matter
        ref, mag = kk.dots(c.V, c.y, c.n_dot, 32, wgt=wgt)
        for k in (1, 9, 32):
            out = c.prob.krylov_op("dots", k, V=c.V[:k], y=c.y)
            _check_sums(f"weighted dots k={k}", out["red"][0, :k], ref[:k], mag[:k])
            s_ref, s_mag, y_ref = kk.dots_fused(c.V[:k], None, c.n_dot, k, c.neq, x0=c.x0, y_index=k - 1, wgt=wgt)
            out = c.prob.krylov_op("dots_fused", k, V=c.V[:k], x0=c.x0, y_index=k - 1)
            _check_sums(f"weighted dots_fused k={k}", out["red"][0, :k], s_ref, s_mag)
        n_ref, n_mag = kk.norm2(c.y, c.n_dot, wgt=wgt)
        _check_sums("weighted norm2", c.prob.krylov_op("norm2", y=c.y, slot=2)["red"][0, 2], n_ref, n_mag)
        # (the Newton loop's norm2_publish stays unweighted on one GPU: its |F| is the unscaled one)
        n_ref, n_mag = kk.norm2(c.y, c.n_dot)
        _check_sums("norm2_publish under scaling", c.prob.krylov_op("norm2_publish", 1, y=c.y)["red"][0, 0], n_ref, n_mag)
        for k in (2, 5, 8):
            w_ref, w_mag, s_ref, s_mag = kk.spmv_dots(c.J, c.x, c.V, c.n_owned, c.neq, k, wgt=wgt)
            out = c.prob.krylov_op("spmv_dots", k, V=c.V[:k - 1], x=c.x, finish=0)
            _check_sums(f"weighted spmv_dots k={k}", out["red"][0, :k], s_ref, s_mag)
            width = int(np.diff(c.J.indptr).max())                         # (w itself is not weighted)
            assert np.all(np.abs(out["y"] - w_ref) <= (width + 2) * EPS * w_mag)
        V, _ = _orthonormal(c, 3)
        red = _pattern()
        red[0, kk.RED_REFINE] = 1.0
        _, _, _, s_ref, s_mag = kk.refine(red, [c.pad(v) for v in V], c.pad(c.y), c.n_dot, 4, wgt=wgt)
        out = c.prob.krylov_op("cgs_refine", 4, V=V, y=c.y, red=red)
        _check_sums("weighted refine", out["red"][1, :3], s_ref[:3], s_mag[:3])
    finally:
        c.prob.set_krylov_scaling("none")


# ---- refusals, and the context afterwards --------------------------------------------------------------------------
def test_bad_arguments_are_hard_errors(contexts):
    a, b, five = contexts("a"), contexts("b"), contexts("five")
    for op, k, kw in (("dots", 0, dict(y=b.y)), ("dots", 33, dict(y=b.y)), ("dots", 5, dict(V=b.V[:4], y=b.y)),
                      ("cgs_update", 31, dict(V=b.V[:30], y=b.y)), ("newton_update", 9, dict(V=b.V[:9], y=b.y, coef=np.ones(9))),
                      ("cgs_update_fs", 5, dict(V=b.V[:5], y=b.y)), ("spmv_dots", 9, dict(V=b.V[:8], x=b.x)),
                      ("spmv_dots", 1, dict(V=b.V[:1], x=b.x)), ("cgs_refine", 6, dict(V=b.V[:5], y=b.y)),
                      ("norm2", 0, dict(y=b.y, slot=40)), ("field_error", 0, dict(y=b.y, x=b.x, slot=3)),
                      ("dots", 2, dict(V=b.V[:2])), ("dots", 2, dict(V=b.V[:2], y=b.y, sentinel=math.inf))):
        with pytest.raises(RuntimeError, match="fedm_debug_krylov_op"):
            b.prob.krylov_op(op, k, **{"V": b.V[:max(k, 1)] if k <= 32 else b.V, **kw})
    with pytest.raises(RuntimeError, match="three equations"):
        five.prob.krylov_op("spmv_dots", 3, V=five.V[:2], x=five.x)
    for op, kw in (("cgs_update_fs", dict(y=five.y)), ("scale_copy_fs", dict(x=five.x)), ("cgs_refine", dict(y=five.y))):
        with pytest.raises(RuntimeError, match="two species"):
            five.prob.krylov_op(op, 2, V=five.V[:2], **kw)
    with pytest.raises(RuntimeError, match="buffers"):                     # two species, but no hierarchy set up
        a.prob.krylov_op("cgs_update_fs", 2, V=a.V[:2], y=a.y)
    out = b.prob.krylov_op("norm2", y=b.y)                                 # a refusal leaves the entry usable
    assert out["host_seq"] == out["device_seq"]


def test_a_linear_solve_afterwards_behaves_as_on_a_fresh_context():
    """Every op on a context, then test_gpu_krylov's solve and its `check`: the steps, the path counters and the
    solution of a context that never saw the entry."""
    import test_gpu_krylov as tk
    fresh, J, F = tk.make_problem("init48")
    used, _, _ = tk.make_problem("init48")
    try:
        b = tk.rhs_of("random", fresh, J, F)
        c = Context("used", used, True)
        first = used.krylov_op("dots", 3, V=c.V[:3], y=c.y, finish=1)
        assert first["allocated"]                                          # the Krylov storage came from the entry
        red = _pattern()
        red[0, kk.RED_REFINE] = 1.0
        used.krylov_op("cgs_refine", 3, V=c.V[:2], y=c.y, red=red)
        used.krylov_op("spmv_dots", 4, V=c.V[:3], x=c.x, finish=2, red=red)
        used.krylov_op("cgs_update_fs", 2, V=c.V[:2], y=c.y, red=red)
        used.krylov_op("newton_update", 2, V=c.V[:2], y=c.y, coef=[0.1, 0.2], finish=1)
        used.krylov_op("field_error", y=c.y, x=c.x, slot=1)
        used.krylov_op("norm2_publish", 3, y=c.y)
        m0 = tk.solve_and_measure(fresh, J, b)
        m1 = tk.solve_and_measure(used, J, b)
        tk.check("fresh context", m0)
        tk.check("after the ops", m1)
        assert m1["its"] == m0["its"] and m1["stats"] == m0["stats"]
        assert np.linalg.norm(m1["x"] - m0["x"]) <= 1e-9 * np.linalg.norm(m0["x"])
        again = used.krylov_op("dots", 3, V=c.V[:3], y=c.y, finish=1)
        assert not again["allocated"] and again["host_seq"] == again["device_seq"] > first["host_seq"]
        assert np.array_equal(again["red"], first["red"])
    finally:
        fresh.close()
        used.close()
