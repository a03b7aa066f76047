"""Regenerate what tests/test_reference_scripts.py holds the own drivers against, from the REFERENCE's three
example scripts (run where the reference checkout is readable; the scripts are read from it at run time and
executed on the fedm_amd facade with their imports redirected, tests/script_harness.py):

* script_records.json -- what each script hands to the device, condensed: the bytes of the fedm_model_desc /
  fedm_gd_desc it lowers to, and per uploaded array its shape, sum, sum of squares and eight strided samples;
* script_records.npz -- the same records whole, small (no pickles; tests/script_harness.py save_records): strings,
  the float arrays packed losslessly, the arrays compared exactly (bytes, indices) as SHA-256 digests;
* script_statements.json -- per script, SHA-256 fingerprints (16 hex digits) of its logical statements, for the
  overlap check against the own drivers.  One-way digests: no statement text is stored.

    python tests/golden/make_script_records.py
"""
import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

import script_harness as sh     # noqa: E402

if __name__ == "__main__":
    full = {case: sh.run_reference_script(case, tempfile.mkdtemp(prefix=f"ref_{case}_")) for case in sh.SCRIPTS}
    records = {case: sh.digest(rec) for case, rec in full.items()}
    (HERE / "script_records.json").write_text(json.dumps(records, separators=(",", ":")) + "\n")
    sh.save_records(HERE / "script_records.npz", full)
    prints = {case: sorted({sh.fingerprint(s) for s in sh.statements(sh.REFERENCE / path)})
              for case, path in sorted(sh.SCRIPTS.items())}
    (HERE / "script_statements.json").write_text(json.dumps(prints, indent=0) + "\n")
    print({k: sorted(v) for k, v in records.items()})
