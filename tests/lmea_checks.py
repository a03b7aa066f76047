"""What the LMEA assembly tests share (helper module of test_gpu_glow_discharge.py, test_gpu_lmea_family.py and
test_lmea_family_reference.py): the two error metrics F and J are held to, and a mirror of the launch plan's LDS
arithmetic (csrc/gd.hip, gd_plan)."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

SLICE = 64                      # cells a workgroup
LDS_TABLE_LIMIT = 80 * 1024     # staged data + table of exponentials: two workgroups in a CU's 160 KiB


def residual_error(F_gpu, F_cpu, n_eq=5):
    """largest error of F relative to the scale of its component"""
    scale = np.abs(F_cpu).reshape(-1, n_eq).max(axis=0)
    return (np.abs(F_gpu - F_cpu).reshape(-1, n_eq) / scale).max()


def jacobian_error(J_gpu, J_cpu):
    """largest error of J relative to the largest entry of its row"""
    rs = np.maximum(abs(J_cpu).max(axis=1).toarray().ravel(), 1e-300)
    return (sp.diags(1.0 / rs) @ abs(J_gpu - J_cpu)).max()


GdLds = namedtuple("GdLds", "staged table exp_table launch")


def gd_lds(n_eq, n_reactions, n_qp):
    """Dynamic LDS of gd_jacobian_rows_kernel: `staged` -- vertex ids, nodal fields and unknowns of 64 cells; `table` --
    exp(u) at the quadrature points, kept (`exp_table`) while staged + table fit 80 KiB; `launch` -- what the launch asks
    for: those and the rows' reaction weights and powers and the sentinel list."""
    from fedm_amd import _lib
    n_fields = 4 * (n_eq - 1) + 2 * n_reactions + 3
    staged = 8 * ((3 * SLICE + 1) // 2 + SLICE * n_fields * 3 + SLICE * 3 * n_eq)
    table = 8 * n_qp * n_eq * SLICE
    exp_table = staged + table <= LDS_TABLE_LIMIT
    launch = staged + (table if exp_table else 0) + (n_eq - 1) * _lib.GD_MAX_REACTIONS * 12 + _lib.GD_MAX_REACTIONS * 4 + 8
    return GdLds(staged, table, exp_table, launch)


def gd_lds_bytes(n_eq, n_reactions, n_qp):
    return gd_lds(n_eq, n_reactions, n_qp).launch
