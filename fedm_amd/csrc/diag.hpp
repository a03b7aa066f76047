// Discharge diagnostics (include/fedm_hip.h, fedm_diagnostics): what the kernels and the C ABI in diag.hip share with
// the context's teardown.
#pragma once
#include "fedm_internal.hpp"

namespace fedm {

// slots of the cell pass's sums: species integrals, the induced current, the groups
constexpr int DIAG_SUM_CURRENT = FEDM_MAX_SPECIES, DIAG_SUM_GROUP0 = FEDM_MAX_SPECIES + 1;
constexpr int DIAG_SUMS = DIAG_SUM_GROUP0 + FEDM_DIAG_MAX_GROUPS;
constexpr int DIAG_CELL_MAXES = 2;   // 0: all cells, 1: the window's

// what the second pass leaves for the one read-back (fedm_diag's fields without its layout promises)
struct DiagResult {
    double sum[DIAG_SUMS];
    double cell_max[DIAG_CELL_MAXES], centroid[DIAG_CELL_MAXES][2];
    double nodal_max[FEDM_MAX_SPECIES];
    int cell[DIAG_CELL_MAXES], vertex[FEDM_MAX_SPECIES];
    int not_finite, pad_;
};

struct Diag {
    double *psi = nullptr;        // [nvp] weighting potential, or null
    int8_t *group = nullptr;      // [nvp] 0 or 1..n_groups, or null
    int n_groups = 0;
    // slot-major partials of the two first passes, one entry per workgroup (postproc.hpp, POST_BLOCKS at the most)
    double *sum_part = nullptr;   // [DIAG_SUMS][POST_BLOCKS]
    double *max_part = nullptr;   // [DIAG_CELL_MAXES + FEDM_MAX_SPECIES][POST_BLOCKS]
    int *idx_part = nullptr;      // the same shape: where each maximum sits
    int *flag_part = nullptr;     // [2][POST_BLOCKS] not-finite flags of the cell and the vertex pass
    DiagResult *result = nullptr;
};

}  // namespace fedm
