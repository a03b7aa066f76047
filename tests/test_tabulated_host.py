"""Host side of the tabulated E/N coefficients (no GPU): the TermSum algebra with table factors, what fill() writes,
fedm.Coefficient_table through the form compiler, the tabulated deck and its generator."""
import ctypes as C
import filecmp
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from fedm_amd import _lib, file_io
from fedm_amd.termsum import TermSum, parse

ROOT = Path(__file__).resolve().parent.parent
DECKS = ROOT / "decks" / "streamer_discharge" / "file_input"
GRID = np.concatenate([np.geomspace(0.05, 40.0, 400), [0.0, 1.0, 2.0, 4.0, 1.5, 3.0, 1e9]])


def _tables():
    t = TermSum.table([1.0, 2.0, 4.0], [1.0, 3.0, 2.0])
    u = TermSum.table([1.5, 3.0, 3.5, 9.0], [0.0, 1.0, -2.0, 5.0])
    return t, u


def test_value_and_derivative_follow_the_lookup_semantics():
    t, _ = _tables()
    assert [t(E) for E in (0.5, 1.0, 1.5, 3.0, 4.0, 7.0)] == [1.0, 1.0, 2.0, 2.5, 2.0, 2.0]
    # the slope of the segment for x[0] <= E < x[n-1] (at a knot: of the segment that begins there), 0 outside
    assert [t.derivative(E) for E in (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 7.0)] == [0.0, 2.0, 2.0, -0.5, -0.5, 0.0, 0.0]
    one = TermSum.table([3.0], [7.0])
    assert one(0.1) == one(3.0) == one(1e9) == 7.0 and one.derivative(3.0) == 0.0
    assert np.isnan(t(float("nan"))) and np.isnan(t.derivative(float("nan")))
    for bad in (([1.0, 1.0], [0.0, 1.0]), ([2.0, 1.0], [0.0, 1.0]), ([], []), ([1.0, np.inf], [0.0, 1.0]),
                ([1.0, 2.0], [0.0, np.nan]), ([1.0, 2.0], [0.0])):
        with pytest.raises(ValueError):
            TermSum.table(*bad)


def test_sum_of_tables_is_exact_on_the_union_grid():
    t, u = _tables()
    s = 2.0 * t - 3.0 * u + 1.0
    assert len(s.tables) == 1 and list(s.tables[0].x) == [1.0, 1.5, 2.0, 3.0, 3.5, 4.0, 9.0]
    eps = np.finfo(float).eps
    for E in GRID:
        # exact in real arithmetic; in floating point a few roundings of the terms that cancel
        size = 2.0 * abs(t(E)) + 3.0 * abs(u(E)) + 1.0
        assert abs(s(E) - (2.0 * t(E) - 3.0 * u(E) + 1.0)) <= 8 * eps * size
    for E in GRID[:400]:        # away from the knots: the derivative too
        assert s.derivative(E) == pytest.approx(2.0 * t.derivative(E) - 3.0 * u.derivative(E), rel=1e-13, abs=1e-14)
    assert (5.0 - t)(3.0) == 2.5 and (t + 0.0)(3.0) == 2.5 and (0.0 + t).tables == t.tables
    assert (t - t)(3.0) == 0.0


def test_products_take_up_to_two_table_factors():
    t, u = _tables()
    g = parse("2.0*E_m**0.5 + 1.0")
    f = g * t * u / 4.0
    assert len(f.tables) == 2
    for E in GRID[:400]:
        assert f(E) == pytest.approx(g(E) * t(E) * u(E) / 4.0, rel=1e-15, abs=1e-300)
        h = 1e-6 * E
        exact = (g.derivative(E) * t(E) * u(E) + g(E) * t.derivative(E) * u(E) + g(E) * t(E) * u.derivative(E)) / 4.0
        assert f.derivative(E) == pytest.approx(exact, rel=1e-13, abs=1e-13)
        if all(abs(E - k) > 2 * h for k in (1.0, 1.5, 2.0, 3.0, 3.5, 4.0, 9.0)):
            assert f.derivative(E) == pytest.approx((f(E + h) - f(E - h)) / (2 * h), rel=1e-5, abs=1e-7)
    assert (-f)(3.2) == -f(3.2) and (f * 0.0).terms == [] and not f.is_const() and not t.is_const()
    assert t.same_as(TermSum.table([1.0, 2.0, 4.0], [1.0, 3.0, 2.0])) and not t.same_as(u)
    # the order in which the factors were multiplied does not make another coefficient, and a zero coefficient
    # carries no factor (it cannot trip the two-factor limit either)
    assert (t * u * g).same_as(u * g * t) and not (t * u * g).same_as(t * t * g)
    zero = t * u * 0.0
    assert zero.tables == () and (zero * t).terms == [] and (zero * t * u).tables == ()


def test_what_the_family_does_not_hold_is_refused_by_name():
    t, u = _tables()
    with pytest.raises(ValueError, match="product of 3 tabulated coefficients"):
        t * u * t
    for make in (lambda: t + parse("E_m"), lambda: t * parse("E_m") + 1.0, lambda: t * u + t, lambda: t * u - 1.0):
        with pytest.raises(ValueError, match="sum with a tabulated coefficient"):
            make()
    for make in (lambda: t ** 2, lambda: 1.0 / t, lambda: parse("E_m") / t, lambda: t ** 0.5):
        with pytest.raises(ValueError, match="power .* of a tabulated coefficient"):
            make()
    with pytest.raises(ValueError, match=r"exp\(\) of a tabulated coefficient"):
        t.exp()
    assert (t ** 1).same_as(t)
    with pytest.raises(TypeError):
        TermSum.coerce(([1.0, 2.0], [3.0, 4.0]))        # a bare (kx, ky) pair is still no coefficient of |E|


def test_fill_writes_the_reference_and_plain_sums_keep_their_bytes():
    t, u = _tables()
    for text in ("2.3987*E_m**(-0.26)", "(1.1944e6 + 4.3666e26 * E_m**(-3))*exp(-2.73e7/E_m)-340.75", "0.0", "7"):
        ts, got, want = parse(text), _lib.TermSumC(), _lib.TermSumC()
        ts.fill(got)
        want.n_terms = len(ts.terms)
        for i, (c, p, q, r) in enumerate(ts.terms):
            want.c[i], want.p[i], want.q[i], want.r[i] = c + 0.0, p + 0.0, q + 0.0, r + 0.0
        assert bytes(got) == bytes(want) and got.pad_ == 0
        tables = []
        ts.fill(got, tables)
        assert bytes(got) == bytes(want) and tables == []
    tables, c1, c2, c3 = [], _lib.TermSumC(), _lib.TermSumC(), _lib.TermSumC()
    (t / 3.0).fill(c1, tables)
    (parse("E_m") * u * TermSum.table([1.0, 2.0, 4.0], [1.0, 3.0, 2.0])).fill(c2, tables)     # u, then an equal of t
    (t * 0.0).fill(c3, tables)
    assert c1.pad_ == 1 and c2.pad_ == (2 | (1 << 16)) and c3.pad_ == 0 and c3.n_terms == 0 and len(tables) == 2
    assert c1.n_terms == 1 and c1.c[0] == 1.0 / 3.0 and c2.p[0] == 1.0
    with pytest.raises(ValueError, match="together with the model's tables"):
        t.fill(_lib.TermSumC())
    many = [TermSum.table([1.0, 2.0], [0.0, float(k)]).tables[0] for k in range(_lib.MAX_TABLES)]
    with pytest.raises(ValueError, match="more than 16 distinct coefficient tables"):
        t.fill(_lib.TermSumC(), many)
    assert C.sizeof(_lib.TermSumC) == 8 + 4 * 8 * _lib.MAX_TERMS          # the layout did not move


def test_binding_names_the_new_entry_point_and_asks_for_a_rebuild_without_it(tmp_path, monkeypatch):
    assert "fedm_ctx_create_tabulated" in _lib.exported_symbols() and _lib.ABI_VERSION == 10
    # a library of the same ABI version without the symbol (what an older build is): refused with the rebuild message
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc")
    src = tmp_path / "old.c"
    src.write_text("int fedm_abi_version(void) { return %d; }\n" % _lib.ABI_VERSION)
    subprocess.run([cc, "-shared", "-fPIC", "-o", str(tmp_path / "libold.so"), str(src)], check=True)
    monkeypatch.setattr(_lib, "LIB_PATH", tmp_path / "libold.so")
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="lacks .*fedm_ctx_create_tabulated.*rebuild it"):
        _lib.load()


def _example():
    spec = importlib.util.spec_from_file_location("streamer_example_tab", ROOT / "examples" / "streamer_discharge.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_coefficient_table_goes_through_the_form_compiler(tmp_path):
    """examples/streamer_discharge.py with the tabulated deck up to the first solve, on the recording stand-in of
    tests/script_harness.py: the descriptor it hands to the device is the case module's, tables included."""
    import script_harness as sh
    import fedm_amd.functions as ff
    from fedm_amd.cases import streamer
    mod = _example()
    with sh._recording(tmp_path) as log:
        with pytest.raises(sh.FirstSolve):
            mod.main(cells=12, output_dir=tmp_path / "out", quiet=True, model="tabulated_model")
    rec = dict(log)
    want = streamer.model_from_deck(model_name="tabulated_model")
    md, ptr, tx, ty = want.to_c_tabulated()
    assert rec["descriptor_type"] == "Model" and rec["descriptor"].tobytes() == bytes(md)
    assert md.mu[1].pad_ == 1 and md.D[1].pad_ == 2 and md.k[0].pad_ == (3 | (1 << 16)) and list(ptr) == [0, 96, 192, 288]
    # the same through the hook the other lowering tests use: the compiled model's tables, array by array
    seen = {}

    class Stop(Exception):
        pass

    def capture(J, F, bcs):
        seen.update(F=F)
        raise Stop
    with pytest.raises(Stop):
        mod.main(cells=12, output_dir=tmp_path / "out2", quiet=True, model="tabulated_model", stop_before_device=capture)
    model, _, _ = ff.compile_forms(seen["F"])
    md2, ptr2, tx2, ty2 = model.to_c_tabulated()
    assert bytes(md2) == bytes(md) and np.array_equal(ptr2, ptr) and np.array_equal(tx2, tx) and np.array_equal(ty2, ty)
    assert tx[0] == pytest.approx(1.0 * streamer.N0 * 1e-21) and np.all(np.diff(tx[:96]) > 0)
    # the default deck is untouched by the model choice
    with pytest.raises(Stop):
        mod.main(cells=12, output_dir=tmp_path / "out3", quiet=True, stop_before_device=capture)
    default, ref = ff.compile_forms(seen["F"])[0], streamer.model()
    assert not default.mu[1].tables and not default.D[1].tables and not default.reactions[0].k.tables
    assert default.mu[1].same_as(ref.mu[1]) and default.D[1].same_as(ref.D[1])
    for E in (1e5, 3e7):
        assert default.reactions[0].k(E) == pytest.approx(ref.reactions[0].k(E), rel=1e-14)
    with pytest.raises(TypeError, match="E_m must be the field magnitude"):
        ff.Coefficient_table(parse("2*E_m"), [1.0, 2.0], [1.0, 2.0], 1e25)
    tab = ff.Coefficient_table(TermSum.field(), [1.0, 10.0], [5.0, 7.0], 2e25)
    assert list(tab.tables[0].x) == [2e4, 2e5] and tab(2e4) == 5.0 and tab(1e9) == 7.0


def test_deck_readers_on_the_tabulated_deck():
    file_io.files.file_input = DECKS
    try:
        n, names, prop_files, _ = file_io.read_speclist(DECKS / "tabulated_model")
        assert n == 3 and names == ["neutrals", "ions", "e"]
        kx, ky, dep = file_io.read_transport_coefficients(names, "mobility", "tabulated_model")
        dx, dy, ddep = file_io.read_transport_coefficients(names, "Diffusion", "tabulated_model")
        e = len(names) - 1
        assert dep[e] == ddep[e] == "E/N" and set(dep[:e]) | set(ddep[:e]) == {"const."}
        assert len(kx[e]) == len(ky[e]) == len(dx[e]) == 96 and kx[e] == dx[e]
        assert kx[e][0] == 1.0 and kx[e][-1] == 1500.0 and np.all(np.diff(kx[e]) > 0)
        alpha = DECKS / "tabulated_model" / "transport_coefficients" / "alpha.dat"
        assert file_io.read_dependence(alpha) == "E/N"
        (ax,), (ay,) = file_io.read_rate_coefficients([alpha], ["E/N"])
        assert ax == kx[e] and len(ay) == 96 and ay[0] < 0.0 < ay[-1]
    finally:
        del file_io.files.__dict__["_dir_file_input"]
    # sampled from the benchmark deck's closed forms: the model agrees with it to the tabulation error of the grid
    from fedm_amd.cases import streamer
    tab, ref = streamer.model_from_deck(model_name="tabulated_model"), streamer.model()
    for E in np.geomspace(5e4, 3e7, 60):
        assert tab.mu[1](E) == pytest.approx(ref.mu[1](E), rel=3e-4)
        assert tab.D[1](E) == pytest.approx(ref.D[1](E), rel=3e-4)
    # ... and exactly (to the ten digits the files hold) at the knots
    for td in kx[e][::7]:
        E = td * streamer.N0 * 1e-21
        assert tab.mu[1](E) == pytest.approx(ref.mu[1](E), rel=1e-9)
        assert tab.D[1](E) == pytest.approx(ref.D[1](E), rel=1e-9)
        assert tab.reactions[0].k(E) == pytest.approx(ref.reactions[0].k(E), rel=1e-8)


def test_generator_reproduces_the_committed_deck(tmp_path):
    spec = importlib.util.spec_from_file_location("make_tabulated_deck", ROOT / "tools" / "make_tabulated_deck.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = gen.write(tmp_path / "tabulated_model")
    committed = DECKS / "tabulated_model"
    names = sorted(p.relative_to(committed) for p in committed.rglob("*") if p.is_file())
    assert names == sorted(p.relative_to(out) for p in out.rglob("*") if p.is_file()) and len(names) == 11
    for name in names:
        assert filecmp.cmp(committed / name, out / name, shallow=False), name
