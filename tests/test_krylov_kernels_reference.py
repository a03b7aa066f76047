"""tests/krylov_kernels_reference.py against independent forms (np.longdouble sums, fractions where a formula is
exact), and its deliberate faults against the bounds tests/test_gpu_krylov_kernels.py holds the device to: every fault
must move the answer by more than 100x its bound (the convention of fieldsplit_reference.PERTURBATIONS).  No GPU."""
import ctypes as C
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import krylov_kernels_reference as kk

ROOT = Path(__file__).resolve().parent.parent
SUM_BOUND = 1e-12           # |sum - fsum| <= SUM_BOUND sum |terms|: tests/test_gpu_diagnostics.py's standing condition
EPS = kk.EPS


def basis(rng, n_vec, n):
    """Pairwise different vectors, entries of magnitude in [0.5, 2] with random signs."""
    return rng.uniform(0.5, 2.0, (n_vec, n)) * rng.choice([-1.0, 1.0], (n_vec, n))


def coefficients(k):
    """Distinct, of order one, no two of them equal in magnitude."""
    return np.array([(-1.0) ** i * (0.3 + 0.07 * i) for i in range(k)])


def update_bound(k, mag):
    return (k + 2) * EPS * mag


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(3)
    n_dot, n, np_ = 700, 760, 832          # owned rows, caller's rows (ghosts behind the owned), padded rows
    V = np.array([kk.padded(v, n_dot, np_) for v in basis(rng, 32, n)])
    y = kk.padded(basis(rng, 1, n)[0], n_dot, np_)
    wgt = kk.padded(rng.uniform(0.1, 3.0, n), n_dot, np_)
    return dict(n_dot=n_dot, n=n, np_=np_, V=V, y=y, wgt=wgt, rng=rng)


# ---- the restatement against independent forms -------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_dots_are_the_longdouble_sums_over_the_owned_rows(small, weighted):
    s = small
    w = s["wgt"] if weighted else None
    got, mag = kk.dots(s["V"], s["y"], s["n_dot"], 32, wgt=w)
    ld = np.longdouble
    for i in range(32):
        terms = s["V"][i, :s["n_dot"]].astype(ld) * s["y"][:s["n_dot"]].astype(ld)
        if weighted:
            terms = terms * s["wgt"][:s["n_dot"]].astype(ld)
        assert abs(ld(got[i]) - terms.sum()) <= 4 * EPS * float(np.abs(terms).sum())
        assert mag[i] == pytest.approx(float(np.abs(terms).sum()), rel=1e-14)
    assert np.isfinite(got).all() and np.abs(got).max() < 1e6      # no sentinel has been read


def test_fused_dots_scatter_x0_and_read_the_new_y(small):
    s = small
    neq, nvert = 5, s["n_dot"] // 5
    x0 = np.full(s["n"] // neq + 1, 1e30)
    x0[:nvert] = basis(np.random.default_rng(4), 1, nvert)[0]
    got, _, y_new = kk.dots_fused(s["V"], None, s["n_dot"], 9, neq, x0=x0, y_index=3)
    expect_y = s["V"][3].copy()
    expect_y[neq - 1:nvert * neq:neq] = x0[:nvert]
    assert np.array_equal(y_new, expect_y)
    assert np.array_equal(y_new[s["n_dot"]:], s["V"][3][s["n_dot"]:])         # nothing behind the owned rows is touched
    for i in range(9):
        xi = expect_y if i == 3 else s["V"][i]
        assert got[i] == pytest.approx(float(np.dot(xi[:s["n_dot"]], expect_y[:s["n_dot"]])), rel=1e-12, abs=1e-9)
    plain, _, y_same = kk.dots_fused(s["V"], s["y"], s["n_dot"], 9, neq)
    assert np.array_equal(y_same, s["y"]) and np.array_equal(plain, kk.dots(s["V"], s["y"], s["n_dot"], 9)[0])


def test_finish_formulae_in_exact_arithmetic():
    h = [0.5, -0.25, 0.125]
    ww = 1.0
    hn2, sound, scale = kk.finish_values(h, ww)
    exact = Fraction(1) - sum(Fraction(v) ** 2 for v in h)
    assert Fraction(hn2) == exact and sound and scale == 1.0 / math.sqrt(hn2)
    assert kk.finish_values([1.0], 1.0) == (0.0, False, 1.0)                      # w in the span of V
    assert kk.finish_values([1.0], 1.0 + 5e-9)[1:] == (False, 1.0)                # below the 1e-8 ww test
    assert kk.finish_values([1.0], 1.0 + 2e-8)[1] is True
    assert kk.finish_values([2.0], 1.0)[1:] == (False, 1.0)                       # hn2 < 0
    before = np.arange(100.0, 100.0 + kk.RED_K)
    sums = np.array([0.5, -0.25, 0.125, 1.0])
    cgs = kk.finish(sums, 4, before, "cgs")
    red = kk.finish(sums, 4, before, "reduce")
    flagged = kk.finish(np.array([1.0, 1.0]), 2, before, "reduce", flag_refine=True)
    for out in (cgs, red):
        assert list(out[:3]) == h and out[3] == hn2 and out[kk.RED_K - 2] == 1.0 and out[kk.RED_K - 1] == scale
        assert out[kk.RED_SPARE] == before[kk.RED_SPARE]
    assert np.array_equal(cgs[4:kk.RED_K - 2], before[4:kk.RED_K - 2])            # in place: the rest stays
    assert not red[4:kk.RED_SPARE].any()                                          # from scratch: the rest is 0
    assert flagged[kk.RED_REFINE] == 1.0 and flagged[kk.RED_K - 1] == 1.0
    assert kk.finish(sums, 4, before, "reduce", flag_refine=True)[kk.RED_REFINE] == 0.0


@pytest.mark.parametrize("k", [1, 7, 8, 9, 17, 30])
def test_updates_are_the_longdouble_updates(small, k):
    s = small
    ld = np.longdouble
    coef = np.zeros(kk.RED_K)
    coef[:k] = coefficients(k)
    coef[kk.RED_K - 1] = 0.37
    got, mag = kk.cgs_update(s["y"], s["V"], coef, k)
    ref = s["y"].astype(ld)
    for i in range(k):
        ref = ref - ld(coef[i]) * s["V"][i].astype(ld)
    ref = ref * ld(0.37)
    assert (np.abs(got.astype(ld) - ref) <= update_bound(k, mag)).all()
    got, mag = kk.multi_axpy(s["y"], s["V"], coef[:k], k, sign=-1.0)
    ref = s["y"].astype(ld)
    for i in range(k):
        ref = ref - ld(coef[i]) * s["V"][i].astype(ld)
    assert (np.abs(got.astype(ld) - ref) <= update_bound(k, mag)).all()
    if k <= 8:
        un, d, mag, mag_d, (dd, _), (uu, _) = kk.newton_update(s["y"], s["V"], coef[:k], k, s["n_dot"])
        ref_d = sum(ld(coef[i]) * s["V"][i].astype(ld) for i in range(k))
        assert (np.abs(d.astype(ld) - ref_d) <= update_bound(k, mag_d)).all()
        assert (np.abs(un.astype(ld) - (s["y"].astype(ld) + ref_d)) <= update_bound(k, mag)).all()
        assert dd == pytest.approx(float((d[:s["n_dot"]].astype(ld) ** 2).sum()), rel=1e-14)
        assert uu == pytest.approx(float((un[:s["n_dot"]].astype(ld) ** 2).sum()), rel=1e-14)


def test_normalise_copy_edges(small):
    x = small["y"]
    assert np.array_equal(kk.normalise_copy(x, 4.0), 0.5 * x)
    for n2 in (0.0, -1.0, math.inf, math.nan, 1.7e308):
        assert not kk.normalise_copy(x, n2).any()


def test_refine_flag_paths(small):
    s = small
    rng = np.random.default_rng(8)
    Q, _ = np.linalg.qr(basis(rng, 4, s["n_dot"]).T)
    V = np.array([kk.padded(q, s["n_dot"], s["np_"]) for q in Q.T])
    t = kk.padded(basis(rng, 1, s["n_dot"])[0], s["n_dot"], s["np_"])
    red = np.zeros((2, kk.RED_K))
    red[0, :4] = [0.1, 0.2, 0.3, 0.4]
    red[0, kk.RED_SPARE] = 7.0
    same, t_same, _, sums, _ = kk.refine(red, V, t, s["n_dot"], 5)
    assert sums is None and np.array_equal(same, red) and np.array_equal(t_same, t)
    red[0, kk.RED_REFINE] = 1.0
    after, t2, _, sums, _ = kk.refine(red, V, t, s["n_dot"], 5)
    assert after[0, kk.RED_REFINE] == 1.0 and after[0, kk.RED_SPARE] == 7.0
    assert np.allclose(after[0, :4], red[0, :4] + sums[:4]) and np.array_equal(after[1, :4], sums[:4])
    assert abs(np.linalg.norm(t2[:s["n_dot"]]) - 1.0) < 1e-12                     # orthonormalised
    assert np.abs(Q.T @ t2[:s["n_dot"]]).max() < 1e-12
    t_in = kk.padded(Q @ np.array([1.0, -2.0, 0.5, 3.0]), s["n_dot"], s["np_"])   # t in the span of V
    after, t3, _, _, _ = kk.refine(red, V, t_in, s["n_dot"], 5)
    assert after[0, kk.RED_REFINE] == 2.0 and after[0, kk.RED_K - 1] == 1.0 and after[1, kk.RED_K - 1] == 1.0


def test_first_stage_and_field_error(small):
    rng = np.random.default_rng(9)
    nv, ns = 50, 2
    t = basis(rng, 1, nv * 3)[0]
    A = rng.uniform(1.0, 2.0, (nv, ns, ns)) + 3.0 * np.eye(ns)
    import scipy.sparse as sp
    J = sp.block_diag([np.block([[A[v], np.ones((ns, 1))], [np.ones((1, ns)), np.ones((1, 1))]]) for v in range(nv)]).tocsr()
    dinv = kk.species_block_inverses(J, nv, ns)
    assert np.allclose(np.einsum("vrc,vcd->vrd", dinv, A), np.eye(ns))
    g, mag, b0 = kk.first_stage(t, dinv, nv, ns)
    for v in (0, 17, 49):
        assert np.allclose(g[v], np.linalg.solve(A[v], t[3 * v:3 * v + 2]), rtol=1e-6)
    assert np.array_equal(b0, t[2::3]) and (mag >= np.abs(g) * (1 - 1e-6)).all()
    u, uo = basis(rng, 2, 60)
    (d, _), (o, _) = kk.field_error(u, uo, 15, 3, 1)                              # 15 owned of 20 vertices
    ld = np.longdouble
    a, b = u[1:45:3].astype(ld), uo[1:45:3].astype(ld)
    assert d == pytest.approx(float(((a - b + ld(3e-16)) ** 2).sum()), rel=1e-14)
    assert o == pytest.approx(float(((b + ld(3e-16)) ** 2).sum()), rel=1e-14)


# ---- every deliberate fault misses its bound by more than 100x -----------------------------------------------------
def _sum_miss(got, ref, mag):
    return np.max(np.abs(np.asarray(got) - np.asarray(ref)) / (SUM_BOUND * np.asarray(mag)))


def test_faults_of_the_sums_miss_the_bound(small):
    s = small
    ref, mag = kk.dots(s["V"], s["y"], s["n_dot"], 17)
    for p in ("last", "range", "chunk_base"):
        got, _ = kk.dots(s["V"], s["y"], s["n_dot"], 17, perturb=p)
        assert _sum_miss(got, ref, mag) > 100.0, p
    # (a dropped entry is 1 / n_dot of sum |terms| at least 0.25 / (4 n_dot): 1e-6 of it at 250 000 entries)
    n2, m2 = kk.norm2(s["y"], s["n_dot"])
    for p in ("last", "range"):
        assert abs(kk.norm2(s["y"], s["n_dot"], perturb=p)[0] - n2) > 100.0 * SUM_BOUND * m2, p
    un, d, _, _, (dd, md), (uu, mu) = kk.newton_update(s["y"], s["V"], coefficients(3), 3, s["n_dot"])
    for p in ("last", "range"):
        _, _, _, _, (dd_p, _), (uu_p, _) = kk.newton_update(s["y"], s["V"], coefficients(3), 3, s["n_dot"], perturb=p)
        assert abs(dd_p - dd) > 100.0 * SUM_BOUND * md and abs(uu_p - uu) > 100.0 * SUM_BOUND * mu, p


def test_a_stride_loop_that_stops_after_one_trip_misses_the_bound():
    rng = np.random.default_rng(5)
    n_dot = kk.RED_BLOCKS * 256 + 1228                        # 210 x 210 vertices, three equations
    V = basis(rng, 2, n_dot)
    ref, mag = kk.dots(V, V[1], n_dot, 2)
    got, _ = kk.dots(V, V[1], n_dot, 2, perturb="stride")
    assert _sum_miss(got, ref, mag) > 100.0
    last, _ = kk.dots(V, V[1], n_dot, 2, perturb="last")       # one entry of 132 300 is still 1e6 bounds
    assert _sum_miss(last, ref, mag) > 100.0


def test_self_index_ignored_after_the_scatter_misses_the_bound(small):
    s = small
    neq, nvert = 5, s["n_dot"] // 5
    x0 = basis(np.random.default_rng(6), 1, s["n"] // neq + 1)[0]
    ref, mag, _ = kk.dots_fused(s["V"], None, s["n_dot"], 9, neq, x0=x0, y_index=8)
    got, _, _ = kk.dots_fused(s["V"], None, s["n_dot"], 9, neq, x0=x0, y_index=8, perturb="self")
    assert abs(got[8] - ref[8]) > 100.0 * SUM_BOUND * mag[8]
    assert np.array_equal(np.delete(got, 8), np.delete(ref, 8))


@pytest.mark.parametrize("k", [9, 16, 17, 30])
def test_faults_of_the_updates_miss_the_bound(small, k):
    s = small
    coef = np.zeros(kk.RED_K)
    coef[:k] = coefficients(k)
    coef[kk.RED_K - 1] = 0.37
    ref, mag = kk.cgs_update(s["y"], s["V"], coef, k)
    for p in ("swap8", "chunk_base", "final_every_chunk"):
        got, _ = kk.cgs_update(s["y"], s["V"], coef, k, perturb=p)
        # (every owned entry, not the worst one: an index mix-up must show wherever the test looks; behind the owned
        # rows all vectors hold the same sentinel, where a swap shows nothing)
        assert (np.abs(got - ref) > 100.0 * update_bound(k, mag))[:s["n_dot"]].all(), p
    ref, mag = kk.multi_axpy(s["y"], s["V"], coef[:k], k)
    for p in ("swap8", "chunk_base"):
        got, _ = kk.multi_axpy(s["y"], s["V"], coef[:k], k, perturb=p)
        assert (np.abs(got - ref) > 100.0 * update_bound(k, mag))[:s["n_dot"]].all(), p


# ---- the binding ---------------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    from fedm_amd import _lib
    from fedm_amd.device import DeviceProblem
    header = (ROOT / "include" / "fedm_hip.h").read_text()
    assert "int fedm_debug_krylov_op(fedm_ctx *ctx, int op, int k, fedm_krylov_io *io);" in header
    assert _lib._SIGNATURES["fedm_debug_krylov_op"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(_lib.KrylovIo)])
    body = re.search(r"typedef struct \{([^}]*)\} fedm_krylov_io;", header).group(1)
    names = [re.sub(r"\[.*\]", "", m) for m in re.findall(r"[\w ]+[ *](\w+(?:\[\d+\])?);", body)]
    assert names == [f[0] for f in _lib.KrylovIo._fields_]
    enum = re.search(r"enum \{\s*(FEDM_KOP_DOTS[^}]*)\}", header).group(1)
    ops = [e.split("=")[0].strip() for e in enum.split(",") if e.strip()]
    assert ops[-1] == "FEDM_KOP_COUNT"
    assert {"FEDM_KOP_" + name.upper(): v for name, v in _lib.KRYLOV_OPS.items()} == {e: i for i, e in enumerate(ops[:-1])}
    assert int(re.search(r"#define FEDM_KOP_RED_K (\d+)", header).group(1)) == _lib.KOP_RED_K == kk.RED_K
    internal = (ROOT / "fedm_amd" / "csrc" / "fedm_internal.hpp").read_text()
    assert f"constexpr int RED_K = {kk.RED_K};" in internal and f"constexpr int RED_BLOCKS = {kk.RED_BLOCKS};" in internal
    assert C.sizeof(_lib.KrylovIo) == 6 * 4 + 2 * 8 + 11 * 8 + 4 * 8
    assert callable(DeviceProblem.krylov_op)
