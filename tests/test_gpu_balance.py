"""The LMEA balance on the device (csrc/gd_balance.hip, DeviceProblem.balance) against the numpy restatement of
tests/balance_reference.py, which tests/test_balance_reference.py pins on the oracle's element residual, and against the
device's own assembled residual.

Meshes of the 1 cm x 1 cm gap: 10 x 10 crossed -- 400 cells, two workgroups of 256, the second with 144, 40 tagged facets
(less than one wave per tag) -- and 129 x 129 crossed -- 66 564 cells, more than BAL_BLOCKS x BAL_THREADS = 65 536, so the
cell pass's stride loop runs, and 516 tagged facets a tag's workgroup walks in three rounds.  States: the perturbed state
of tests/test_gpu_glow_discharge.py::_reference (u_new != u_old != u_old1, dt != dt_old).  Deck and sentinel losses;
axisymmetric and planar.  psi = z / gap + 0.2 (r / gap)^2 has both gradient components.

Bounds.  Sums: |device - fsum| <= 1e-12 sum |terms| of the restatement (tests/test_gpu_diagnostics.py's bound).  The
identity: the downloaded residual summed per component against Balance.imbalance within 1e-11 sum |terms| of the row (the
residual's own parity bound against the oracle).  Field maximum 1e-13 relative, cell and centroid exact where the
restatement's maximum is unique.  Nodal maxima bitwise.  Every figure is printed before it is asserted.
"""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import balance_reference as bref  # noqa: E402
import test_balance_reference as tb  # noqa: E402

pytestmark = pytest.mark.gpu
SUM_BOUND, IDENTITY_BOUND, MAX_BOUND = 1e-12, 1e-11, 1e-13
GAP = 0.01


def _psi(coords):
    return coords[:, 1] / GAP + 0.2 * (coords[:, 0] / GAP) ** 2


def _electrodes(coords):
    z = coords[:, 1]
    return np.where(np.abs(z) < 3e-16, 1, np.where(np.abs(z - GAP) < 3e-16, 2, 0)).astype(np.int8)


class Case:
    """One (mesh, losses, geometry): the oracle's model and fields, the states, the restatement (computed once, never
    changed) and one device problem with psi and the electrode groups set up."""

    def __init__(self, n, losses, planar):
        from oracle import gd as ogd
        from fedm_amd.device import DeviceProblem
        if n == 10:
            c = tb.perturbed_case(losses)
        else:
            o = ogd.GlowDischarge(tb.DECK, n, n)
            if losses == "sentinels":
                o.deck.energy_loss, o.deck.energy_Ei = list(tb.SENTINEL_LOSSES), 15.76
            nv = o.mesh.nv
            rng = np.random.default_rng(1)
            me_old = 3.0 + rng.normal(0, 0.3, nv)
            me = me_old + rng.normal(0, 0.05, nv)
            U = np.zeros((nv, 5))
            U[:, 1:4] = np.log(1e12) + rng.normal(0, 0.2, (nv, 3))
            U[:, 0] = np.log(me) + U[:, 3] + rng.normal(0, 0.05, nv)
            U[:, 4] = -100.0 * (1 - o.mesh.coords[:, 1] / GAP) + rng.normal(0, 0.02, nv)
            co = o.coefficients(me_old, np.abs(rng.normal(30.0, 5.0, nv)))
            Uo, Uo1 = U + rng.normal(0, 0.02, U.shape), U + rng.normal(0, 0.02, U.shape)
            import types
            c = types.SimpleNamespace(o=o, U=U, Uo=Uo, Uo1=Uo1, co=co, me_old=me_old, me=me, dt=1.1e-12, dt_old=0.7e-12,
                                      fields=tb.field_table(co, me_old, me, Uo[:, 3]))
        self.c, self.o = c, c.o
        o = c.o
        self.model = tb.oracle_model(o, axisymmetric=not planar)
        self.psi, self.group = _psi(o.mesh.coords), _electrodes(o.mesh.coords)
        self.prob = DeviceProblem(o.mesh.coords, o.mesh.cells, self.model, facet_tags=o.tags,
                                  dirichlet_dofs=o.dirichlet_dofs, dirichlet_vals=o.dirichlet_values(2e-12))
        self.prob.set_gd_fields(c.fields)
        self.prob.set_state(c.U, c.Uo, c.Uo1)
        self.prob.set_step(c.dt, c.dt_old)
        self.prob.balance_setup(weighting_potential=self.psi, vertex_groups=self.group, n_groups=2)
        self.ref = tb.restate(c, self.model.to_c(), psi=self.psi, group=self.group, n_groups=2)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n=10, losses="deck", planar=False):
        if (n, losses, planar) not in made:
            made[n, losses, planar] = Case(n, losses, planar)
        return made[n, losses, planar]
    yield get
    for c in made.values():
        c.prob.close()


def _pairs(b, ref):
    ns, nr, nt = len(ref["content"]), len(ref["reaction"]), len(ref["wall"])
    pairs = [(f"content[{c}]", b.content[c], ref["content"][c]) for c in range(ns)]
    pairs += [(f"rate[{c}]", b.rate_of_change[c], ref["rate_of_change"][c]) for c in range(ns)]
    pairs += [(f"reaction[{j}]", b.reaction[j], ref["reaction"][j]) for j in range(nr)]
    pairs += [("collision_loss", b.collision_loss, ref["collision_loss"]), ("joule", b.joule, ref["joule"]),
              ("I_psi", b.induced_current, ref["induced_current"])]
    pairs += [(f"wall[{t}][{c}]", b.wall[t, c], ref["wall"][t][c]) for t in range(nt) for c in range(ns)]
    pairs += [(f"ion_flux[{t}]", b.ion_flux[t], ref["ion_flux"][t]) for t in range(nt)]
    pairs += [(f"q[{g}]", b.group_sum[g], r) for g, r in enumerate(ref["group_sum"])]
    return pairs


def _check_sums(what, b, ref):
    ratios, spread = {}, {}
    for name, got, r in _pairs(b, ref):
        ratios[name] = abs(got - r.value) / r.abs if r.abs > 0.0 else (0.0 if got == 0.0 else math.inf)
        spread[name] = abs(r.plain - r.value) / r.abs if r.abs > 0.0 else 0.0
    print(f"[balance] {what}: |device - fsum| / sum|terms| " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()), flush=True)
    print(f"[balance] {what}: |plain float64 order - fsum| / sum|terms|, worst {max(spread.values()):.2e}", flush=True)
    assert b.finite
    assert len(b.group_sum) == len(ref["group_sum"])
    for name, v in ratios.items():
        assert v <= SUM_BOUND, (what, name, v)


def _check_maxima(what, b, ref, U):
    r = ref["field"]
    print(f"[balance] {what}: field max rel {abs(b.field_max - r.value) / r.value:.2e} cell {b.field_max_cell} restated "
          f"{r.index} unique {r.unique}", flush=True)
    assert abs(b.field_max - r.value) <= MAX_BOUND * r.value
    if r.unique:
        assert b.field_max_cell == r.index and tuple(b.field_max_centroid) == r.centroid
    ns = U.shape[1] - 1
    for c, rn in enumerate(ref["nodal"]):
        assert b.nodal_max[c] == rn.value, (what, c)                     # bitwise
        v = b.nodal_max_vertex[c]
        assert (U[v, c] if c < ns else U[v, 0] - U[v, ns - 1]) == rn.value, (what, c)
        if rn.unique:
            assert v == rn.index, (what, c)
    assert b.mean_energy_max == float(np.exp(ref["nodal"][ns].value))      # (numpy's exp: the dataclass's)


def _check_identity(what, prob, b, ref):
    F, _ = prob.residual()
    rows = F.reshape(-1, prob.n_eq)
    for c, imb in enumerate(bref.imbalance(ref)):
        got = math.fsum(rows[:, c].tolist())
        ratio = abs(got - b.imbalance[c]) / imb.abs
        print(f"[balance] {what}: row {c} sum of F {got:.6e} imbalance {b.imbalance[c]:.6e} restated {imb.value:.6e} "
              f"|difference| / sum|terms| {ratio:.2e}", flush=True)
        assert ratio <= IDENTITY_BOUND, (what, c, ratio)


def _bytes(b):
    parts = [b.content, b.rate_of_change, b.reaction, np.array([b.collision_loss, b.joule, b.induced_current, b.field_max]),
             b.wall, b.ion_flux, b.group_sum, np.array(b.field_max_centroid), b.nodal_max,
             np.array([b.field_max_cell, int(b.finite)]), b.nodal_max_vertex]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


@pytest.mark.parametrize("n,losses,planar", [(10, "deck", False), (10, "sentinels", False), (10, "deck", True),
                                             (10, "sentinels", True), (129, "deck", False), (129, "sentinels", True)])
def test_sums_maxima_and_the_identity(cases, n, losses, planar):
    c = cases(n, losses, planar)
    what = f"{n} x {n} {losses} {'planar' if planar else 'axisymmetric'}"
    if n == 129:
        assert c.o.mesh.nc == 66564 > 256 * 256
    b = c.prob.balance()
    _check_sums(what, b, c.ref)
    _check_maxima(what, b, c.ref, c.c.U)
    _check_identity(what, c.prob, b, c.ref)
    ref = c.ref
    assert ref["induced_current"].value != 0.0 and ref["group_sum"][0].abs > 0.0 and ref["group_sum"][1].abs > 0.0
    # the derived fields are the caller's arithmetic on the raw ones
    from fedm_amd.physical_constants import elementary_charge, epsilon_0
    assert np.array_equal(b.surface_charge, epsilon_0 * b.group_sum) and b.current == elementary_charge * b.induced_current
    assert b.power_joule == elementary_charge * b.joule and b.source[0] == b.joule - b.collision_loss
    assert np.array_equal(b.wall_current, elementary_charge * (b.wall[:, 2] - b.wall[:, 3]))
    # tags 3 and 4 reflect everything and emit nothing: exactly 0, also on the axis where r = 0
    assert np.array_equal(b.wall[2:], np.zeros((2, 4))) and np.all(b.wall[:2, 1:] != 0.0) and np.all(b.wall[:, 0] == b.wall[:, 0])


def test_two_calls_agree_byte_for_byte_and_nothing_is_touched(cases):
    c = cases(129, "deck", False)
    F0, _ = c.prob.residual()
    U0, f0 = c.prob.get_state(), c.prob.get_gd_fields()
    first = c.prob.balance()
    assert _bytes(c.prob.balance()) == _bytes(first)
    assert np.array_equal(c.prob.get_state(), U0) and np.array_equal(c.prob.get_state_old(), c.c.Uo)
    assert np.array_equal(c.prob.get_gd_fields(), f0)
    F1, _ = c.prob.residual()
    # (the default residual goes through the element buffer and a gather in a fixed order: the same bits)
    assert np.array_equal(F1, F0)
    assert _bytes(c.prob.balance()) == _bytes(first)


def test_a_nan_is_flagged_and_the_next_call_is_clean(cases):
    c = cases(10, "deck", False)
    first = c.prob.balance()
    try:
        bad = c.c.U.copy()
        bad[c.o.mesh.nv // 2 + 5, 1] = np.nan
        c.prob.set_state(u_new=bad)
        assert c.prob.balance().finite is False          # returns: the kernels read and reduce the NaN, nothing faults
        bad = c.c.U.copy()
        bad[3, 4] = np.inf                               # ... and an infinite potential
        c.prob.set_state(u_new=bad)
        assert c.prob.balance().finite is False
    finally:
        c.prob.set_state(u_new=c.c.U)
    again = c.prob.balance()
    assert again.finite is True and _bytes(again) == _bytes(first)


def test_without_a_setup_there_is_no_current_and_no_group(cases):
    from fedm_amd.device import DeviceProblem
    c = cases(10, "deck", False)
    o = c.o
    prob = DeviceProblem(o.mesh.coords, o.mesh.cells, c.model, facet_tags=o.tags, dirichlet_dofs=o.dirichlet_dofs,
                         dirichlet_vals=o.dirichlet_values(2e-12))
    try:
        prob.set_gd_fields(c.c.fields)
        prob.set_state(c.c.U, c.c.Uo, c.c.Uo1)
        prob.set_step(c.c.dt, c.c.dt_old)
        b, full = prob.balance(), c.prob.balance()
        assert b.induced_current == 0.0 and b.group_sum.size == 0 and b.finite
        assert np.array_equal(b.content, full.content) and np.array_equal(b.wall, full.wall)
        assert np.array_equal(b.reaction, full.reaction) and b.joule == full.joule
    finally:
        prob.close()


def test_refusals_through_the_c_abi(cases):
    from fedm_amd import _lib
    from fedm_amd.cases import streamer
    c = cases(10, "deck", False)
    lib, h = c.prob.lib, c.prob._h
    out = _lib.GdBalanceOut()
    nv = c.prob.nv
    grp = np.zeros(nv, dtype=np.int8)
    gp = grp.ctypes.data_as(C.POINTER(C.c_int8))
    assert lib.fedm_gd_balance(h, None) == -2 and "null" in _lib.last_error()
    assert lib.fedm_gd_balance_setup(h, None, gp, 9) == -2 and "9 groups" in _lib.last_error()
    assert lib.fedm_gd_balance_setup(h, None, None, 2) == -2 and "array" in _lib.last_error()
    grp[5] = 3
    assert lib.fedm_gd_balance_setup(h, None, gp, 2) == -2 and "group[5] = 3" in _lib.last_error()
    psi = np.zeros(nv)
    psi[7] = np.inf
    assert lib.fedm_gd_balance_setup(h, psi.ctypes.data_as(C.POINTER(C.c_double)), None, 0) == -2
    assert "psi[7]" in _lib.last_error()
    # a refused set-up leaves the earlier one in place
    assert _bytes(c.prob.balance()) == _bytes(c.prob.balance()) and c.prob.balance().group_sum.size == 2
    m = streamer.mesh(4)
    lfa = streamer.device_problem(m.coords, m.cells)
    try:
        assert lib.fedm_gd_balance(lfa._h, C.byref(out)) == -2 and "LFA context" in _lib.last_error()
        assert lib.fedm_gd_balance_setup(lfa._h, None, None, 0) == -2 and "LFA context" in _lib.last_error()
        with pytest.raises(RuntimeError, match="LMEA models only"):
            lfa.balance()
    finally:
        lfa.close()


def test_a_context_with_ghosts_is_refused(cases):
    """The last three vertices of the 10 x 10 mesh as ghosts of a rank that owns the rest (the way
    tests/test_gpu_diagnostics.py makes a rank's context on one GPU): the balance has no owned-share weighting and
    refuses the context, set-up and call alike."""
    from fedm_amd import _lib
    from fedm_amd.device import DeviceProblem
    c = cases(10, "deck", False)
    o = c.o
    prob = DeviceProblem(o.mesh.coords, o.mesh.cells, c.model, facet_tags=o.tags, dirichlet_dofs=o.dirichlet_dofs,
                         dirichlet_vals=o.dirichlet_values(2e-12), n_owned=o.mesh.nv - 3)
    try:
        out = _lib.GdBalanceOut()
        assert prob.lib.fedm_gd_balance(prob._h, C.byref(out)) == -2 and "ghost" in _lib.last_error()
        assert prob.lib.fedm_gd_balance_setup(prob._h, None, None, 0) == -2 and "ghost" in _lib.last_error()
        with pytest.raises(RuntimeError, match="ghost"):
            prob.balance()
    finally:
        prob.close()


def _example():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gd_example_balance", tb.ROOT / "examples" / "glow_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_rows_are_the_facades_and_the_cases(tmp_path):
    """examples/glow_discharge.py --balance on an 8 x 8 mesh over three accepted steps: every row is, to the last bit,
    the Balance the device problem returned at that moment; the facade called again after the run returns the last
    one; and Case.balance() -- our own set-up of the same model -- with the example's last states, field table and step
    sizes copied onto its device problem returns the same row within the sums' bound."""
    from fedm_amd import functions as ff
    from fedm_amd.cases import glow_discharge as gdc
    mod = _example()
    seen = dict(problem=None, balances=[], old=[], steps=[])

    def build(J, F, bcs):
        p = ff.Problem(J, F, bcs)
        asked, set_step = p.device.balance, p.device.set_step

        def recording():
            b = asked()
            seen["balances"].append(b)
            seen["old"].append(p.device.get_state_old())
            return b

        def stepping(dt, dt_old):
            seen["steps"].append((dt, dt_old))
            return set_step(dt, dt_old)
        p.device.balance, p.device.set_step = recording, stepping
        seen["problem"] = p
        return p
    out = tmp_path / "balance.txt"
    res = mod.main(nx=8, ny=8, T_final=1e-11, output_dir=tmp_path, stop_before_device=build, balance=out)
    names = open(out).readline().split()[1:]
    rows = np.loadtxt(out).reshape(-1, len(names))
    assert names == mod.balance_columns(res["species"]) and len(names) == 1 + 4 + 4 + 4 + 1
    assert rows.shape[0] == res["steps"] == len(seen["balances"]) >= 3
    for k, b in enumerate(seen["balances"]):
        assert b.finite
        assert np.array_equal(rows[k, 1:], np.array(mod.balance_row(0.0, b)[1:], dtype=np.float64)), k
    assert rows[-1, 0] == res["t"] and np.all(np.diff(rows[:, 0]) > 0.0)
    dev = seen["problem"].device
    del dev.balance, dev.set_step
    psi = dev.coords[:, 1] / mod.GAP
    again = ff.Discharge_balance(seen["problem"], boundary_tags=(1, 2), weighting_potential=psi)()
    assert _bytes(again) == _bytes(seen["balances"][-1])
    case = gdc.Case(nx=8, ny=8, device_pipeline=False)
    try:
        assert np.array_equal(case.mesh.cells, dev.cells) and np.array_equal(case.mesh.coords, dev.coords)
        case.prob.set_gd_fields(dev.get_gd_fields())
        case.prob.set_state(dev.get_state(), seen["old"][-1], seen["old"][-2])
        case.prob.set_step(*seen["steps"][-1])
        mine = case.balance()
        # the example lowers its forms to the device model, the Case writes the descriptor by hand: the two agree to
        # rounding (thermal velocities and the like are formed by different expressions), so the rows agree to the
        # sums' bound and not to the bit; the imbalance is a difference, held on the scale of what it is made of
        scale = np.abs(again.rate_of_change) + np.abs(again.source) + np.abs(again.wall).sum(axis=0)
        a, b = np.array(mod.balance_row(0.0, again)[1:]), np.array(mod.balance_row(0.0, mine)[1:])
        unit = np.abs(a)
        unit[8:12] = scale          # the four imbalance columns
        print(f"[balance] example row against Case.balance(): |difference| / scale {np.abs(a - b) / unit}", flush=True)
        assert np.all(np.abs(a - b) <= SUM_BOUND * unit)
        assert np.array_equal(mine.nodal_max, again.nodal_max) and mine.field_max_cell == again.field_max_cell
    finally:
        case.prob.close()


def test_example_without_the_option_writes_the_same_log(tmp_path):
    """The run's own outputs do not depend on the option: `relative error.log` of a run with --balance and of one
    without are the same bytes (the balance touches no state), and no balance file appears without it."""
    mod = _example()
    logs = []
    for name, opt in (("plain", None), ("with", tmp_path / "rows.txt")):
        out = tmp_path / name
        mod.main(nx=8, ny=8, T_final=1e-11, output_dir=out, balance=opt)
        logs.append((out / "relative error.log").read_bytes())
        assert sorted(p.name for p in out.iterdir()) == sorted(p.name for p in (tmp_path / "plain").iterdir())
    assert logs[0] == logs[1] and len(logs[0]) > 0
    assert (tmp_path / "rows.txt").exists() and not list((tmp_path / "plain").glob("*rows*"))


def test_case_keeps_the_balance_of_the_step_it_solved():
    """keep_balance=True: last_balance is taken between the solve and the mean-energy update.  A call after step() sees
    the next step's mean-energy field: contents and reaction totals are the same bits, the electrons' wall terms move."""
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=16, ny=16, T_final=1.0, keep_balance=True)
    for _ in range(3):
        case.step()
    kept, after = case.last_balance, case.balance()
    assert kept.finite and after.finite
    assert np.array_equal(kept.content, after.content) and np.array_equal(kept.reaction, after.reaction)
    assert np.array_equal(kept.wall[:, 1:3], after.wall[:, 1:3]) and not np.array_equal(kept.wall[:, 3], after.wall[:, 3])
    scale = np.abs(kept.rate_of_change) + np.abs(kept.source) + np.abs(kept.wall).sum(axis=0)
    print(f"[balance] Case, in the step: imbalance / (|rate| + |source| + |walls|) {np.abs(kept.imbalance) / scale}; "
          f"after it {np.abs(after.imbalance) / scale}", flush=True)
    case.prob.close()


def test_case_balance_after_a_step():
    """fedm_amd.cases.glow_discharge.Case.balance() after accepted steps of the device pipeline: set up at the first call,
    the electrodes' groups and psi = z / gap (the mean-energy field is the next step's by then); the imbalance against its terms is printed, not bounded (the Newton solve
    stops on the 2-norm of F, which does not bound the rows' sums)."""
    from fedm_amd.cases import glow_discharge as gdc
    case = gdc.Case(nx=16, ny=16, T_final=1.0)
    for _ in range(3):
        case.step()
    b = case.balance()
    assert b.finite and b.group_sum.size == 2 and b.induced_current != 0.0
    assert np.all(b.content > 0.0) and b.field_max > 0.0 and b.mean_energy_max > 0.0
    scale = np.abs(b.rate_of_change) + np.abs(b.source) + np.abs(b.wall).sum(axis=0)
    print(f"[balance] Case after 3 steps: imbalance / (|rate| + |source| + |walls|) {np.abs(b.imbalance) / scale}", flush=True)
    assert _bytes(case.balance()) == _bytes(b)
