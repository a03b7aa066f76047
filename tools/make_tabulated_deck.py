#!/usr/bin/env python3
"""Writes decks/streamer_discharge/file_input/tabulated_model: the benchmark model with the electrons' mobility and
diffusion coefficient and the ionisation coefficient as two-column `Dependence: E/N` tables, the way a Boltzmann
solver delivers them.  The tables are SAMPLED FROM THE BENCHMARK DECK'S OWN CLOSED FORMS (benchmark_model/
transport_coefficients/{e_Nb,e_ND,alpha}.dat, Bagheri et al. 2018) on one log-spaced E/N grid, so a run with them
differs from the closed-form deck by the tabulation error alone.  Everything else is copied from benchmark_model.

    python tools/make_tabulated_deck.py [--out DIR] [--knots N]

tests/test_tabulated_host.py (test_generator_reproduces_the_committed_deck) checks that this script reproduces the committed files byte for byte.
"""
import argparse
import shutil
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from fedm_amd.cases.streamer import N0      # noqa: E402  (gas number density [1/m^3] at 760 Torr, 300 K)

TD_LO, TD_HI, KNOTS = 1.0, 1500.0, 96       # E/N grid [Td]: 2.4e4 .. 3.7e7 V/m, beyond what the streamer head reaches

HEADER = """################################################################################
#
# Description: {what}
# {subject}
# Data source: sampled from benchmark_model/transport_coefficients/{src} (B. Bagheri Plasma Sources Sci. Technol. 27 (2018) 095002)
# Data:        E/N [Td]  {unit}
# Dependence:  E/N
# Comment:     N0 = {n0:.4e} 1/m^3; written by tools/make_tabulated_deck.py
#
################################################################################

"""


def tables(knots=KNOTS):
    """(E/N [Td], N0 * mu_e, N0 * D_e, alpha / N0) from the benchmark deck's closed forms."""
    from fedm_amd import file_io
    from fedm_amd.termsum import parse
    src = ROOT / "decks" / "streamer_discharge" / "file_input" / "benchmark_model" / "transport_coefficients"
    mu, D, alpha = (parse(file_io.read_single_string(src / name)) for name in ("e_Nb.dat", "e_ND.dat", "alpha.dat"))
    td = np.array([float(f"{v:.5E}") for v in np.geomspace(TD_LO, TD_HI, knots)])     # as the files will hold them
    E = td * N0 * 1e-21
    return (td, np.array([N0 * mu(e) for e in E]), np.array([N0 * D(e) for e in E]),
            np.array([alpha(e) / N0 for e in E]))


def write(out, knots=KNOTS):
    out = Path(out)
    base = ROOT / "decks" / "streamer_discharge" / "file_input" / "benchmark_model"
    if out.exists():
        shutil.rmtree(out)
    shutil.copytree(base, out)
    td, nmu, nD, alpha_n = tables(knots)
    files = [("e_Nb.dat", "mobility", "Species:     electrons (field)", "N*b [1/(m*V*s)]", nmu),
             ("e_ND.dat", "diffusion coefficient", "Species:     electrons (field)", "N*D [1/(m*s)]", nD),
             ("alpha.dat", "net ionization coefficient over the gas density",
              "Reaction:    neutrals + e -> ions + e + e", "alpha/N [m^2]", alpha_n)]
    for name, what, subject, unit, y in files:
        text = HEADER.format(what=what, subject=subject, src=name, unit=unit, n0=N0)
        text += "".join(f"{a:.5E}    {b:.9E}\n" for a, b in zip(td, y))
        (out / "transport_coefficients" / name).write_text(text)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "decks" / "streamer_discharge" / "file_input" / "tabulated_model"))
    ap.add_argument("--knots", type=int, default=KNOTS)
    args = ap.parse_args()
    print(write(args.out, args.knots))
