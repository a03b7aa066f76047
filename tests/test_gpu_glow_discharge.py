"""Glow discharge (LMEA, 5 equations) on the device against the oracle and the reference's
own goldens (tests/integrated_tests/glow_discharge/test_glow_discharge.py:48-62)."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from lmea_checks import gd_lds_bytes as _gd_lds_bytes  # noqa: E402
from lmea_checks import jacobian_error as _jacobian_error, residual_error as _residual_error  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DECK = ROOT / "decks" / "glow_discharge" / "file_input" / "4_particles"


SENTINEL_LOSSES = [11.55, 7.77e77, -11.55, 4.21, -7.34, 0.0, 9.99e99]


# fedm_launched_assembly's names (fedm_amd.device._VARIANTS) of the element kernels FEDM_GD_HAND selects
LAUNCHED = {"0": "lmea/dual-number colours", "2": "lmea/atomics", "4": "lmea/element buffer, cell order",
            "3": "lmea/element buffer, destination order",
            "5": "lmea/element buffer, destination order, columns side by side"}
_REFERENCE = {}


def _reference(case, losses="deck", degree=4):
    """The oracle's F and J at a perturbed state of the 10 x 10 crossed mesh (221 vertices, 400 cells: seven workgroups
    of 64 cells, the last with 16, and a position count that is no multiple of 256), with the state and the nodal
    fields they were computed from.  Computed once per (losses, quadrature degree) and read-only from then on."""
    from oracle import gd as ogd
    from oracle.quadrature import interval_rule, triangle_rule
    if (losses, degree) in _REFERENCE:
        return _REFERENCE[losses, degree]
    o = ogd.GlowDischarge(DECK, 10, 10)
    o.xq, o.wq = triangle_rule(degree)       # (nothing else in the oracle depends on the rule)
    o.tq, o.wt = interval_rule(degree)
    if losses == "sentinels":
        o.deck.energy_loss, o.deck.energy_Ei = list(SENTINEL_LOSSES), 15.76
    nv = o.mesh.nv
    rng = np.random.default_rng(0)
    me_old = 3.0 + rng.normal(0, 0.3, nv)
    me = me_old + rng.normal(0, 0.05, nv)
    U = case.U.copy()
    U[:, 0] = np.log(me) + U[:, 3] + rng.normal(0, 0.05, nv)
    U[:, 1:4] += rng.normal(0, 0.2, (nv, 3))
    U[:, 4] = -100.0 * (1 - o.mesh.coords[:, 1] / 0.01) + rng.normal(0, 3.0, nv)
    Uo = U + rng.normal(0, 0.02, U.shape)
    Uo1 = U + rng.normal(0, 0.02, U.shape)
    redE = o.reduced_field(U[:, 4])
    co = o.coefficients(me_old, redE)
    t, dt, dt_old = 2e-12, 1.1e-12, 0.7e-12
    F_cpu, J_cpu = o.residual_jacobian(U, Uo, Uo1, dt, dt_old, co, me_old, me, Uo[:, 3], o.dirichlet_values(t))
    ref = dict(cells=o.mesh.cells, me_old=me_old, me=me, U=U, Uo=Uo, Uo1=Uo1, redE=redE, co=co, t=t, dt=dt,
               dt_old=dt_old, F=F_cpu, J=J_cpu)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REFERENCE[losses, degree] = ref
    return ref


def _upload(case, ref):
    """The reference's state and nodal fields through the product pipeline onto the case's device problem."""
    from fedm_amd import functions as ff
    assert np.array_equal(ref["cells"], case.mesh.cells)
    assert np.allclose(case.project_reduced_field(ref["U"][:, 4]), ref["redE"], rtol=1e-12)
    case.mean_energy_old.vector()[:] = ref["me_old"]
    case.mean_energy.vector()[:] = ref["me"]
    case.redE.vector()[:] = ref["redE"]
    ff.Transport_coefficient_interpolation("update", case.mu_dep, case.N0, case.Tgas, case.mu, case.mu_x,
                                           case.mu_y, case.mean_energy_old, case.redE)
    ff.Transport_coefficient_interpolation("update", case.D_dep, case.N0, case.Tgas, case.D, case.D_x,
                                           case.D_y, case.mean_energy_old, case.redE, case.mu)
    ff.Rate_coefficient_interpolation("update", case.k_dep, case.k, case.k_x, case.k_y,
                                      case.mean_energy_old, case.redE, Te=0, Tgas=0)
    co = ref["co"]
    for a, b in zip(case.mu + case.D + case.k, co["mu"] + co["D"] + co["k"]):
        assert np.allclose(a.vector(), b, rtol=1e-14, atol=0)
    case.U = ref["Uo"].copy()            # u_e_old field = old electron log density
    case.upload_fields()
    prob = case.prob
    prob.set_state(ref["U"], ref["Uo"], ref["Uo1"])
    prob.set_step(ref["dt"], ref["dt_old"])
    prob.set_dirichlet_values(case.dirichlet_values(ref["t"]))
    return prob


@pytest.mark.parametrize("losses", ["deck", "sentinels"])
@pytest.mark.parametrize("variant", ["5", "3", "4", "2", "0"])
def test_gd_residual_and_jacobian_match_the_oracle(variant, losses, monkeypatch):
    """LMEA element Jacobian against the oracle for the device variants (csrc/gd.hip): hand-derived blocks with
    the three column vertices side by side at one wave per SIMD (5), one column vertex per pass (3), both
    through the element buffer in the order of their destinations + gather, the buffer in cell
    order (4, round 2's layout), the same blocks added with atomics (2), and the dual-number kernel (0) that
    cross-checks the hand derivation.  "sentinels": the ionisation loses Ei - mean energy and the elastic collisions
    the mean energy itself, as the decks' sentinel loss values ask (fedm/functions.py:906-909), with the mean-energy
    argument the scripts pass, u[0] / u[n - 1] -- two more columns in the energy row's derivative.
    The launch record says which element kernel ran: the variant of FEDM_GD_HAND, one launch over the seven workgroups
    of 64 cells (a launch per colour for the dual-number kernel), a wave per species/energy row -- or, for variant 5
    under FEDM_GD_WAVES=two, the two-wave workgroups that large meshes get (two rows a wave in turn)."""
    from fedm_amd.cases import glow_discharge as gdc
    monkeypatch.setenv("FEDM_GD_HAND", variant)
    monkeypatch.setenv("FEDM_GD_WAVES", "two" if losses == "sentinels" else "auto")
    extra = dict(energy_loss=SENTINEL_LOSSES, energy_Ei=15.76) if losses == "sentinels" else {}
    case = gdc.Case(nx=10, ny=10, device_pipeline=False, **extra)
    ref = _reference(case, losses)
    prob = _upload(case, ref)
    F_gpu, _ = prob.residual()
    assert _residual_error(F_gpu, ref["F"]) < 1e-11
    prob.jacobian()
    J_gpu = prob.jacobian_csr()
    assert _jacobian_error(J_gpu, ref["J"]) < 1e-9
    rec = prob.launched_assembly()
    n_colours = prob.sizes()["n_colours"]       # (greedy colouring: none of them is empty)
    for what in ("residual", "jacobian"):
        assert rec[what]["variant"] == LAUNCHED[variant], (what, rec)
        assert rec[what]["launches"] == (n_colours if variant == "0" else 1), (what, rec)
        if variant != "0":
            two_waves = what == "jacobian" and variant == "5" and losses == "sentinels"
            assert rec[what]["threads"] == (128 if two_waves else 256), (what, rec)
            assert rec[what]["workgroups"] == 7, (what, rec)


@pytest.mark.parametrize("variant", ["5", "3"])
def test_gd_gathers_per_position_and_per_row_agree_bit_for_bit(variant, monkeypatch):
    """The element buffer in destination order is summed into the matrix by a thread per stored position
    (FEDM_GD_GATHER=positions, gd_gather_dest_kernel) or per (stored position, equation row) (rows, the default,
    gd_gather_dest_rows_kernel).  Both add a position's contributions in list order, so J -- and F, which neither
    touches -- are the same bits; "positions" is also held to the oracle.
    The launch record names the element kernel only, so nothing here shows WHICH gather ran: that "positions" reaches
    gd_gather_dest_kernel rests on the first letter of FEDM_GD_GATHER as csrc/context.cpp reads it (anything but 'r')."""
    from fedm_amd.cases import glow_discharge as gdc
    monkeypatch.setenv("FEDM_GD_HAND", variant)
    out = {}
    for gather in ("positions", "rows"):
        monkeypatch.setenv("FEDM_GD_GATHER", gather)
        case = gdc.Case(nx=10, ny=10, device_pipeline=False)
        ref = _reference(case)
        prob = _upload(case, ref)
        F_gpu, _ = prob.residual()
        prob.jacobian()
        assert prob.launched_assembly()["jacobian"]["variant"] == LAUNCHED[variant]
        out[gather] = (F_gpu, prob.residual_vector(), prob.jacobian_csr())
        prob.close()
    assert _residual_error(out["positions"][0], ref["F"]) < 1e-11
    assert _residual_error(out["positions"][1], ref["F"]) < 1e-11
    assert _jacobian_error(out["positions"][2], ref["J"]) < 1e-9
    assert np.array_equal(out["positions"][0], out["rows"][0])
    assert np.array_equal(out["positions"][1], out["rows"][1])
    Jp, Jr = out["positions"][2], out["rows"][2]
    assert np.array_equal(Jp.indptr, Jr.indptr) and np.array_equal(Jp.indices, Jr.indices)
    assert np.array_equal(Jp.data, Jr.data)


def test_gd_second_context_with_a_larger_lds_need():
    """Dynamic LDS beyond 64 KiB is opt-in per kernel.  The element kernel's need depends on the model (fields,
    quadrature points), not on the mesh: a degree-2 case (3 points, 67 656 bytes) and then, in the same process, a
    degree-4 case (6 points, 75 336 bytes) -- the second needs a larger grant than the first one set.  Both against
    the oracle with its rule at the same degree.  (A refused launch is an error on the host and leaves F zero.)"""
    from fedm_amd import quadrature
    from fedm_amd.cases import glow_discharge as gdc
    needs = []
    for degree in (2, 4):
        case = gdc.Case(nx=10, ny=10, device_pipeline=False, quadrature_degree=degree)
        ref = _reference(case, degree=degree)
        prob = _upload(case, ref)
        needs.append(_gd_lds_bytes(5, prob.model.n_reactions, len(quadrature.triangle(degree)[1])))
        F_gpu, _ = prob.residual()
        f_err = _residual_error(F_gpu, ref["F"])
        prob.jacobian()
        j_err = _jacobian_error(prob.jacobian_csr(), ref["J"])
        fj_err = _residual_error(prob.residual_vector(), ref["F"])
        print(f"degree {degree}: LDS {needs[-1]} bytes, F {f_err:.2e}, F of F + J {fj_err:.2e}, J {j_err:.2e}")
        assert f_err < 1e-11 and fj_err < 1e-11, degree
        assert j_err < 1e-9, degree
        prob.close()
    assert needs == [67656, 75336]
    assert 64 * 1024 < needs[0] < needs[1]


@pytest.mark.parametrize("cg", ["one launch", "launches"])
def test_gd_device_pipeline_matches_host_pipeline(cg, monkeypatch):
    """fedm-gd.py:424-443,452 on the device (projection CG, np.interp look-ups, ESR, mean
    energy) against the same steps with the façade's host functions.  cg: the projection's Jacobi-CG as ONE launch of
    a resident grid with counter barriers (the default for meshes of this size) and launch by launch with its scalars
    on the device (FEDM_GD_CG=launches: larger meshes, and where a barrier of the single launch should ever give up)."""
    from fedm_amd.cases import glow_discharge as gdc
    monkeypatch.setenv("FEDM_GD_CG", "launches" if cg == "launches" else "one")
    host = gdc.Case(nx=24, ny=24, device_pipeline=False, T_final=1.0)
    dev = gdc.Case(nx=24, ny=24, device_pipeline=True, T_final=1.0)
    # A self-comparison of two PIPELINES, so the solves in between must not add a Krylov-path dependent
    # difference of their own: Newton to 1e-12 and GMRES to 1e-13 pin every step's state to a few hundred
    # ulp whatever the path (at the script's tolerances, 1e-4 / 1e-5, rounding-level input differences come
    # back as 1e-12 .. 1e-9: what round 3's widened 1e-8 papered over).  What is left is the pipelines' own
    # disagreement -- table look-ups and products (a few ulp), the projection's Jacobi-CG against a sparse LU
    # (stopped at 1e-13) -- times the condition of a step, bounded here by 1e-10.
    for case in (host, dev):
        case.solver.parameters["relative_tolerance"] = 1e-12
        case.solver.parameters["krylov_relative_tolerance"] = 1e-13
    worst = 0.0
    for _ in range(4):
        host.step()
        dev.step()
        fh, fd = host.prob.get_gd_fields(), dev.prob.get_gd_fields()
        fh[-2] = host.mean_energy.vector()     # the host uploads this row before the next solve
        scale = np.maximum(np.abs(fh).max(axis=1, keepdims=True), 1e-300)
        worst = max(worst, (np.abs(fh - fd) / scale).max())
    print(f"host pipeline vs device pipeline, nodal fields over 4 steps: {worst:.2e}")
    assert worst < 1e-10
    assert np.allclose(host.prob.get_state(), dev.prob.get_state(), rtol=1e-10, atol=1e-10)
    assert np.allclose(np.loadtxt(host.error_file), np.loadtxt(dev.error_file), rtol=1e-8)


@pytest.mark.parametrize("device_pipeline", [False, True])
def test_gd_golden_run(golden_dir, device_pipeline, tmp_path):
    from fedm_amd import mesh_io
    from fedm_amd.cases import glow_discharge as gdc
    gold = np.load(golden_dir / "gd_golden.npz")
    ref_log = np.array(json.loads((golden_dir / "error_logs.json").read_text())["glow_discharge"])
    out = gdc.Case(device_pipeline=device_pipeline).run()
    log = np.array(out["log"])
    assert log.shape == ref_log.shape
    assert np.allclose(log, ref_log)                  # the reference's assertion (rtol 1e-5)
    for key, comp in (("electrons", 3), ("Ar_plus", 2), ("Ar_star", 1)):
        ref = gold[key + "_1"]
        err = (out["snapshot"][:, comp] - ref) / ref
        assert np.mean(np.abs(err)) < 1e-5 and np.sqrt(np.mean(err ** 2)) < 1e-5
        assert np.max(np.abs(err)) < 1e-3
        # the same check the way the reference's test does it: through the XDMF/HDF5 checkpoint
        # (tests/integrated_tests/glow_discharge/test_glow_discharge.py, testing_utils.py:21-24)
        from fedm_amd.mesh import Mesh
        f = mesh_io.XDMFFile(tmp_path / f"{key}.xdmf", Mesh(gold["coords"], gold["cells"]))
        f.write_checkpoint(np.zeros(len(ref)), key, 0.0)        # snapshot _0 (initial condition slot)
        f.write_checkpoint(out["snapshot"][:, comp], key, 1e-11)
        vec = mesh_io.read_h5(tmp_path / f"{key}.h5", key)[1][:, 0]
        rel = (vec - ref) / ref
        assert np.mean(np.abs(rel)) < 1e-5 and np.sqrt(np.mean(rel ** 2)) < 1e-5


def test_glow_discharge_example_writes_the_reference_outputs(tmp_path, golden_dir):
    """examples/glow_discharge.py is our own driver for the case of the reference's fedm-gd.py (deck
    readers -> semi_implicit_coefficients -> Flux -> Source_term / Energy_Source_term -> weak forms ->
    Boundary_flux('flux source') -> Problem -> adaptive_solver -> file_output) on the facade;
    tests/test_reference_scripts.py shows that it hands the device what the reference's script does.  The
    LMEA form is lowered onto the device model by fedm_amd.lmea, the per-step coefficient refresh
    runs on the host through the facade's interpolation functions like in the reference.  The
    run must pass the reference's own assertions (tests/integrated_tests/glow_discharge/
    test_glow_discharge.py:48-62): the six-row error log and the species snapshots at 1e-11 s read
    back from the XDMF/HDF5 checkpoints."""
    import importlib.util
    from fedm_amd import mesh_io
    root = golden_dir.parent.parent
    spec = importlib.util.spec_from_file_location("gd_example", root / "examples" / "glow_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(output_dir=tmp_path)
    assert res["problem"].device.model.n_eq == 5
    gold = np.load(golden_dir / "gd_golden.npz")
    ref_log = np.array(json.loads((golden_dir / "error_logs.json").read_text())["glow_discharge"])
    assert np.allclose(np.loadtxt(tmp_path / "relative error.log"), ref_log)
    for key in ("electrons", "Ar_plus", "Ar_star"):
        vecs = mesh_io.read_h5(tmp_path / "number density" / key / f"{key}.h5", key)
        assert len(vecs) == 2                                  # _0 initial condition, _1 at 1e-11 s
        assert np.allclose(vecs[0][:, 0], np.log(1e12), rtol=1e-14)
        rel = (vecs[1][:, 0] - gold[key + "_1"]) / gold[key + "_1"]
        assert np.mean(np.abs(rel)) < 1e-5 and np.sqrt(np.mean(rel ** 2)) < 1e-5 and np.max(np.abs(rel)) < 1e-3
    assert (tmp_path / "potential" / "Phi" / "Phi.pvd").exists()


def test_glow_discharge_at_200k_dofs_jacobian_is_the_derivative_of_the_residual():
    """BASELINE configs[2] at its full size (141x141 crossed, 200 225 DOFs): the oracle is too slow
    there, so size-independent properties are checked -- the assembled Jacobian is the directional
    derivative of the assembled residual, and a time step of the device pipeline is accepted."""
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=141, ny=141, T_final=1.0)
    prob = case.prob
    assert prob.n == 200225
    for _ in range(2):
        case.step()
    assert case.t > 0 and len(open(case.error_file).readlines()) >= 2
    U = prob.get_state()
    Uo = prob.get_state_old()
    rng = np.random.default_rng(5)
    V = rng.standard_normal(U.shape) * np.array([1e-3, 1e-3, 1e-3, 1e-3, 1e-2])
    prob.set_step(case.dt.time_step, case.dt_old.time_step)
    prob.jacobian()
    Jv = prob.spmv(V.ravel())
    eps = 1e-4
    prob.set_state(U + eps * V)
    Fp, _ = prob.residual()
    prob.set_state(U - eps * V)
    Fm, _ = prob.residual()
    fd = (Fp - Fm) / (2 * eps)
    scale = np.abs(Jv).reshape(-1, 5).max(axis=0)
    assert (np.abs(fd - Jv).reshape(-1, 5) / scale).max() < 1e-5
