"""fedm_amd/csrc/table_lookup.h, the look-up the LFA element kernels use for tabulated coefficients, compiled by the
host compiler into a stand-alone program (tests/table_lookup_main.cpp) and held to np.interp and to the stated
derivative: the segment's slope for x[0] <= E < x[n-1], exactly 0 outside and for one knot; NaN gives NaN; the
segment index stays in [0, max(n - 2, 0)] for any argument."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lookup(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the look-up program with")
    exe = tmp_path_factory.mktemp("table_lookup") / "table_lookup"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'fedm_amd' / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tests" / "table_lookup_main.cpp")], check=True)

    def run(x, y, E):
        fmt = lambda a: " ".join(float(v).hex() for v in a)
        text = f"{len(x)}\n{fmt(x)}\n{fmt(y)}\n{len(E)}\n{fmt(E)}\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split()
        seg = np.array([int(v) for v in out[0::3]])
        val = np.array([float.fromhex(v) for v in out[1::3]])
        der = np.array([float.fromhex(v) for v in out[2::3]])
        return seg, val, der
    return run


def _expected(x, y, E):
    x, y, E = np.asarray(x, float), np.asarray(y, float), np.asarray(E, float)
    with np.errstate(invalid="ignore"):
        val = np.interp(E, x, y)
        der = np.zeros_like(E)
        if x.size >= 2:
            slope = np.diff(y) / np.diff(x)
            j = np.clip(np.searchsorted(x, E, side="right") - 1, 0, x.size - 2)
            der = np.where((E >= x[0]) & (E < x[-1]), slope[j], 0.0)
    nan = np.isnan(E)
    return np.where(nan, np.nan, val), np.where(nan, np.nan, der)


SPECIAL = [0.0, -0.0, -1.0, -1e300, 1e300, 5e-324, np.inf, -np.inf, np.nan]


@pytest.mark.parametrize("n", [1, 2, 3, 9, 64, 257])
def test_value_and_derivative_against_numpy(lookup, n):
    rng = np.random.default_rng(n)
    x = np.cumsum(rng.uniform(0.1, 2.0, n)) * 1e5
    y = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4)
    inside = rng.uniform(x[0] * 0.5, x[-1] * 1.5, 400)
    nextafter = np.concatenate([np.nextafter(x, np.inf), np.nextafter(x, -np.inf)])
    E = np.concatenate([inside, x, nextafter, SPECIAL])
    seg, val, der = lookup(x, y, E)
    assert seg.min() >= 0 and seg.max() <= max(n - 2, 0)
    ev, ed = _expected(x, y, E)
    assert np.array_equal(np.isnan(val), np.isnan(E)) and np.array_equal(np.isnan(der), np.isnan(E))
    ok = ~np.isnan(E)
    # np.interp evaluates slope * (E - x[j]) + y[j] as this header does: equal up to the last bits of the sum
    assert np.allclose(val[ok], ev[ok], rtol=0.0, atol=4 * np.finfo(float).eps * np.abs(y).max())
    assert np.array_equal(der[ok], ed[ok])
    # the ends and the knots exactly: y's own entries, the slope of the segment that begins at the knot, 0 at the last
    k_seg, k_val, k_der = lookup(x, y, x)
    assert np.array_equal(k_val, y)
    if n >= 2:
        assert np.array_equal(k_der[:-1], np.diff(y) / np.diff(x)) and k_der[-1] == 0.0
        assert np.array_equal(k_seg, np.minimum(np.arange(n), n - 2))
    else:
        assert k_der[0] == 0.0
    below, above = lookup(x, y, [x[0] - 1.0, -np.inf]), lookup(x, y, [x[-1] + 1.0, np.inf])
    assert np.all(below[1] == y[0]) and np.all(below[2] == 0.0)
    assert np.all(above[1] == y[-1]) and np.all(above[2] == 0.0)


def test_segment_is_where_the_argument_lies(lookup):
    x = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    y = np.array([0.0, 1.0, 0.0, 3.0, -1.0])
    E = np.array([1.0, 1.5, 2.0, 3.999, 4.0, 7.0, 8.0, 15.9])
    seg, _, _ = lookup(x, y, E)
    assert list(seg) == [0, 0, 1, 1, 2, 2, 3, 3]
