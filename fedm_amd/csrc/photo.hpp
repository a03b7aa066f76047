// Photoionisation in the Helmholtz approximation (include/fedm_hip.h, fedm_photo_setup): what photo.hip (kernels and
// launchers) and photo_abi.cpp (the C ABI) share.  The terms are solved by scalar_cg.hpp's conjugate gradients.
#pragma once
#include "scalar_cg.hpp"

namespace fedm {

constexpr int PHOTO_MAX_TERMS = 4;

struct Photo {
    fedm_photo_desc desc{};
    // per term: the operator K_w + kappa^2 M_w in double precision (what CG multiplies by) and its preconditioner:
    // a hierarchy of plain V(nu,nu) cycles, or null for Jacobi (A's own diagonal)
    EllMat A[PHOTO_MAX_TERMS];
    Amg *M[PHOTO_MAX_TERMS] = {nullptr, nullptr, nullptr, nullptr};
    double *y = nullptr;          // [n_terms][nvp], kept between updates: the next one starts from it
    double *g = nullptr;          // [nvp] load vector
    double *cell_g = nullptr;     // [nc][3] the cells' local load vectors
    int *v_ptr = nullptr;         // [nv + 1] vertex -> its (cell, corner) pairs, ascending: the order of the sum
    int *v_idx = nullptr;         // cell * 3 + corner
    unsigned char *zero = nullptr;   // [nvp] 1: a vertex of a zero-tag facet
    ScalarCgWork cg;              // the solves' scratch
    int64_t stats[8] = {};        // fedm_photo_stats' order
};
enum PhotoStat { PH_UPDATES = 0, PH_CG_ITS0 = 1, PH_VCYCLES = 5, PH_EXHAUSTED = 6 };

// photo.hip
void launch_photo_load_vector(Ctx &c);   // Photo::g from c.d_uold
void launch_photo_table_write(Ctx &c);   // the targets' c.d_ext from Photo::y

}  // namespace fedm
