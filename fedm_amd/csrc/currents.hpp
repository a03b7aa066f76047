// Electrode currents (include/fedm_hip.h, fedm_currents_setup / fedm_currents_solve / fedm_currents): what the kernels
// and the C ABI in currents.hip share with the context's teardown.
#pragma once
#include "photo.hpp"

namespace fedm {

constexpr int CUR_MAX = FEDM_CURRENTS_MAX;
// slots of the cell pass's sums: a row of CUR_MAX per quantity
constexpr int CUR_COND = 0, CUR_DISP = CUR_MAX, CUR_COUP = 2 * CUR_MAX, CUR_CHARGE = 3 * CUR_MAX;
constexpr int CUR_SUMS = 4 * CUR_MAX;

// what the one-workgroup finish leaves for the one read-back
struct CurResult {
    double sum[CUR_SUMS];
    int not_finite, pad_;
};

struct Currents {
    int n_psi = 0;
    double *psi = nullptr;        // [CUR_MAX][nvp] the installed weighting potentials (padding stays 0)
    double cap[CUR_MAX][CUR_MAX] = {};   // the capacitance matrix of the installed potentials
    // slot-major partials of the cell pass, one entry per workgroup (postproc.hpp, POST_BLOCKS at the most)
    double *sum_part = nullptr;   // [CUR_SUMS][POST_BLOCKS]
    int *flag_part = nullptr;     // [POST_BLOCKS]
    CurResult *result = nullptr;
    // fedm_currents_solve (allocated at its first call): the candidates, one system and the vectors scalar_pcg borrows
    double *psi_new = nullptr;    // [CUR_MAX][nvp]
    double *rhs = nullptr;        // [CUR_MAX][nvp] the caller's right-hand sides
    double *x = nullptr, *b = nullptr;   // [nvp] the free vertices' values and their right-hand side (0 on the unit rows)
    unsigned char *fixed = nullptr;      // [nvp] 1: a unit row of the operator (a conductor's vertex), and the padding
    Photo *cg = nullptr;          // r, z, p, q, partials, red alone: Ctx::photo points here for the duration of a solve
};

}  // namespace fedm
