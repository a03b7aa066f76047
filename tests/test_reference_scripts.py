"""Drop-in evidence for the facade (level 1) without shipping the reference's text.

* The reference's three example scripts were run AS WRITTEN on the facade -- their ``from dolfin import *`` /
  ``from fedm.<module> import *`` lines pointed at ``fedm_amd`` -- up to their first nonlinear solve against a
  recording stand-in for the device (tests/script_harness.py), by tests/golden/make_script_records.py: what they
  handed over (mesh, `fedm_model_desc` / `fedm_gd_desc` bytes, Dirichlet rows, the three states, the LMEA nodal
  field table, the source Expression's device program, the step sizes) is stored in tests/golden/script_records.npz
  (float arrays losslessly, the arrays compared exactly as SHA-256 digests) and condensed in
  tests/golden/script_records.json.
* Our own drivers under ``examples/`` must reproduce that record, digest by digest and array by array; tests/
  test_gpu_*.py then hold their runs against the reference's goldens.
* The own drivers are not re-typings of the reference's scripts: statement overlap below 30 %, counted against
  fingerprints of the reference's statements (tests/golden/script_statements.json).
"""
import json
from pathlib import Path

import numpy as np
import pytest

import script_harness as sh

CASES = sorted(sh.SCRIPTS)
GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURE = GOLDEN / "script_records.json"


@pytest.fixture(scope="module")
def fixture_records():
    return json.loads(FIXTURE.read_text())


@pytest.fixture(scope="module")
def own_records(tmp_path_factory):
    return {case: sh.run_own_example(case, tmp_path_factory.mktemp(f"own_{case}")) for case in CASES}


@pytest.mark.parametrize("case", CASES)
def test_own_driver_hands_the_device_what_the_reference_script_does(case, own_records, fixture_records):
    sh.assert_same_digest(sh.digest(own_records[case]), fixture_records[case])


@pytest.mark.parametrize("case", CASES)
def test_reference_script_runs_on_the_facade_as_written(case, own_records, fixture_records):
    """The record of the reference's script run as written on the facade (stored by
    tests/golden/make_script_records.py) against its digest and, array by array, against the own driver's."""
    ref = sh.load_records(GOLDEN / "script_records.npz", case)
    assert sorted(ref) == sorted(fixture_records[case])
    stored = {k: v for k, v in ref.items() if not isinstance(v, sh.Exact)}
    sh.assert_same_digest(sh.digest(stored), {k: fixture_records[case][k] for k in stored})
    own = own_records[case]
    assert sorted(ref) == sorted(own)
    for key, value in ref.items():
        if isinstance(value, str):
            assert own[key] == value
        elif isinstance(value, sh.Exact):
            assert value.matches(own[key]), key                               # bytes and indices: exact
        else:
            np.testing.assert_allclose(own[key], value, rtol=1e-13, atol=0, err_msg=key)


@pytest.mark.parametrize("case", CASES)
def test_own_driver_is_not_the_reference_script_retyped(case):
    name = {"streamer": "streamer_discharge"}.get(case, case)
    own = sh.statements(sh.ROOT / "examples" / f"{name}.py")
    ref = set(json.loads((GOLDEN / "script_statements.json").read_text())[case])
    shared = sum(1 for s in own if sh.fingerprint(s) in ref)
    assert shared < 0.3 * len(own), f"{shared} of {len(own)} statements are the reference's"
    assert shared < 0.3 * len(ref)
