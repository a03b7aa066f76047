"""Row-equilibrated GMRES (``fedm_set_krylov_scaling``), no GPU: the binding, the definition of the scaling, and what
the float64 restatement (tests/scaled_krylov_reference.py) says about the two orders of the field split on the oracle's
Jacobians of ``streamer.mesh(48, 4.0)`` -- the initial state ("init48") and the developed head ("head48"), the recipe of
``table_systems`` in tests/test_krylov_reference.py.

"scaled residual" below is ``|D (J x - b)| / |D b|`` in float64.  Found with this restatement (emulated preconditioner,
V(1,1), degree-6 species polynomial) on head48:

    order, norm tested      ksp_rtol            steps        scaled residual
    lower, unscaled         1e-5                9            8.1e-3
    upper, unscaled         1e-4                3            11.2          <- code 0, 11 times the residual of x = 0
    lower, scaled           1e-4 / 1e-5 / 1e-7  12 / 13 / 17 3.5e-5 / 8.9e-6 / 3.6e-8
    upper, scaled           1e-4 / 1e-5 / 1e-7  12 / 13 / 17 3.9e-5 / 9.9e-6 / 4.0e-8
    scaled, M^-1 applied to v instead of D^-1 v: no convergence in 200 steps
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import krylov_reference as kr
import scaled_krylov_reference as skr
from fieldsplit_reference import FieldSplit, Multigrid

ROOT = Path(__file__).resolve().parent.parent


# ---- the binding ---------------------------------------------------------------------------------------------------
def test_abi_version_and_the_two_entry_points():
    import __graft_entry__ as entry
    entry.build()
    from fedm_amd import _lib
    header = (ROOT / "include" / "fedm_hip.h").read_text()
    lib = _lib.load()
    assert lib.fedm_abi_version() == int(re.search(r"#define FEDM_ABI_VERSION (\d+)", header).group(1)) \
        == _lib.ABI_VERSION == 10
    # the prototypes the header declares are the ones the binding attaches
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int fedm_set_krylov_scaling(fedm_ctx *ctx, int mode);" in flat
    assert "int fedm_get_krylov_scaling(fedm_ctx *ctx, int *mode, double *d_out);" in flat
    sig = dict(_lib._SIGNATURES)
    assert sig["fedm_set_krylov_scaling"] == (C.c_int, [C.c_void_p, C.c_int])
    res, args = sig["fedm_get_krylov_scaling"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1] is C.POINTER(C.c_int) and args[2] is C.POINTER(C.c_double)
    for name in ("fedm_set_krylov_scaling", "fedm_get_krylov_scaling"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == sig[name][1]


def test_facade_parameter_and_device_methods_exist():
    from fedm_amd.device import DeviceProblem
    from fedm_amd.functions import PETScSNESSolver
    assert PETScSNESSolver().parameters["krylov_residual_scaling"] == "none"
    assert callable(DeviceProblem.set_krylov_scaling) and callable(DeviceProblem.krylov_scaling)


# ---- the scaling ---------------------------------------------------------------------------------------------------
def test_row_scale_definition():
    rng = np.random.default_rng(3)
    nv, neq = 40, 3
    n = nv * neq
    J = sp.random(n, n, density=0.1, random_state=7, format="lil")
    for v in range(nv):
        J[v * neq:(v + 1) * neq, v * neq:(v + 1) * neq] = rng.standard_normal((neq, neq)) * 10.0 ** rng.integers(-3, 20)
    identity_rows = [4, 5, 17, 60]
    for i in identity_rows:
        J[i, :] = 0.0
        J[i, i] = 1.0
    zero_row = 31                                    # a row whose entries in the diagonal block are all zero
    J[zero_row, (zero_row // neq) * neq:(zero_row // neq + 1) * neq] = 0.0
    J = sp.csr_matrix(J)
    d = skr.row_scale(J, neq)
    assert np.all(d[identity_rows] == 1.0) and d[zero_row] == 1.0
    blocks = skr.diagonal_blocks(J, neq)
    i = 7
    assert d[i] == 1.0 / np.sqrt((blocks[i // neq, i % neq] ** 2).sum())
    # scaling J's rows by a known diagonal scales s by it (powers of two: exactly)
    g = 2.0 ** rng.integers(-30, 30, n)
    s, sg = skr.row_norms(J, neq), skr.row_norms(sp.diags(g) @ J, neq)
    assert np.array_equal(sg, g * s)
    g = np.exp(rng.standard_normal(n))
    assert np.allclose(skr.row_norms(sp.diags(g) @ J, neq), g * s, rtol=8 * np.finfo(float).eps, atol=0)
    # not finite -> 1
    Jn = J.tolil()
    Jn[9, 9] = np.inf
    Jn[12, 12] = np.nan
    dn = skr.row_scale(sp.csr_matrix(Jn), neq)
    assert dn[9] == 1.0 and dn[12] == 1.0


# ---- the table -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def systems():
    """name -> (J, F, {order: field split}, d) of the oracle on ``streamer.mesh(48, 4.0)``."""
    from fedm_amd import amg
    from fedm_amd.cases import streamer
    from fedm_amd.device import chebyshev_weights
    from oracle import streamer as ost
    from oracle.mesh import Mesh as OMesh
    from test_gpu_preconditioner import _head_state
    from test_krylov_reference import _StateRecorder
    msh = streamer.mesh(48, 4.0)
    om = ost.build(OMesh(msh.coords, msh.cells))
    nv = msh.coords.shape[0]
    out = {}
    for name in ("init48", "head48"):
        if name == "init48":
            U0 = ost.initial_state(om)
            states, step = (U0, U0, U0), (5e-12, 1e30)
        else:
            rec = _StateRecorder(nv)
            _head_state(rec, msh.coords)
            states, step = rec.states, rec.step
        F, J = om.residual_jacobian(*states, *step)
        J = sp.csr_matrix(J)
        fixed = np.zeros(nv, dtype=bool)
        fixed[np.asarray(om.dirichlet_dofs) // 3] = True
        K = J[2::3][:, 2::3].tolil()
        for i in np.nonzero(fixed)[0]:
            K[i, :] = 0.0
            K[:, i] = 0.0
            K[i, i] = 1.0
        levels = amg.build_hierarchy(sp.csr_matrix(K), theta=0.08, max_coarse=40, fixed=fixed, coords=msh.coords)
        mg = Multigrid(levels, nu=1, omega=0.85)
        fs = {o: FieldSplit(J, 2, mg, chebyshev_weights(6), order=o) for o in ("lower", "upper")}
        out[name] = (J, np.asarray(F).ravel(), fs, skr.row_scale(J, 3), np.asarray(om.dirichlet_dofs))
    return out


def _emulated(fs):
    return lambda t: fs.apply(t, "emulate")


def test_scaling_of_the_developed_head(systems):
    J, F, fs, d, ddofs = systems["head48"]
    s = 1.0 / d
    print(f"[scaling] head48 s: species {s.reshape(-1, 3)[:, :2].min():.3e} .. {s.reshape(-1, 3)[:, :2].max():.3e}, "
          f"potential {s[2::3].min():.3e} .. {s[2::3].max():.3e}")
    assert np.all(np.isfinite(d)) and np.all(d > 0.0)
    assert np.all(d[ddofs] == 1.0)                      # Dirichlet rows are identity rows
    # the species rows are some 1e15 times the potential's; in the scaled norm the Poisson rows carry most of |D b|
    assert s.reshape(-1, 3)[:, :2].min() > 1e10 > 1e3 > s[2::3].max()
    Db = d * F
    assert np.linalg.norm(Db[2::3]) > 0.9 * np.linalg.norm(Db)


@pytest.mark.parametrize("rtol", [1e-4, 1e-5, 1e-7])
@pytest.mark.parametrize("order", ["lower", "upper"])
def test_scaled_solves_hold_the_scaled_residual(systems, order, rtol):
    J, F, fs, d, _ = systems["head48"]
    res = skr.scaled_gmres(J, -F, _emulated(fs[order]), d, rtol=rtol, max_it=200)
    true, bnorm = skr.scaled_residual(J, res.x, -F, d)
    print(f"[scaling] head48 {order} scaled {rtol}: {res} scaled residual {true / bnorm:.3e}")
    assert res.code == kr.CONVERGED
    assert true / bnorm <= rtol * (1 + 1e-6)


@pytest.mark.parametrize("order", ["lower", "upper"])
def test_scaled_solve_of_the_early_system(systems, order):
    J, F, fs, d, _ = systems["init48"]
    res = skr.scaled_gmres(J, -F, _emulated(fs[order]), d, rtol=1e-5, max_it=200)
    true, bnorm = skr.scaled_residual(J, res.x, -F, d)
    print(f"[scaling] init48 {order} scaled 1e-5: {res} scaled residual {true / bnorm:.3e}")
    assert res.code == kr.CONVERGED and true / bnorm <= 1e-5 * (1 + 1e-6)
    assert res.its <= 8                                  # the fused-update path of the device


def test_unscaled_upper_order_passes_while_wrong(systems):
    """The hazard the feature removes, kept as a negative control: potential first, unscaled test, ksp_rtol 1e-4 --
    CONVERGED with a scaled residual above that of x = 0 (found: 11.2)."""
    J, F, fs, d, _ = systems["head48"]
    res = kr.gmres(J, -F, _emulated(fs["upper"]), rtol=1e-4, max_it=200)
    true, bnorm = skr.scaled_residual(J, res.x, -F, d)
    print(f"[scaling] head48 upper unscaled 1e-4: {res} scaled residual {true / bnorm:.3e}")
    assert res.code == kr.CONVERGED
    assert true / bnorm >= 100 * 1e-4


@pytest.mark.parametrize("order", ["lower", "upper"])
def test_misformulated_scaling_does_not_converge(systems, order):
    """Rows of the operator scaled, the preconditioner's input not un-scaled: D J M^-1 ~ D."""
    J, F, fs, d, _ = systems["head48"]
    res = skr.scaled_gmres(J, -F, _emulated(fs[order]), d, misformulated=True, rtol=1e-5, max_it=200)
    true, bnorm = skr.scaled_residual(J, res.x, -F, d)
    print(f"[scaling] head48 {order} mis-formulated: {res} scaled residual {true / bnorm:.3e}")
    assert res.code == kr.DIVERGED_LINEAR and res.its == 200
    assert true / bnorm > 1e-5
