// Photoionisation in the Helmholtz approximation (include/fedm_hip.h, fedm_photo_setup): what photo.hip (kernels,
// launchers, the scalar CG) and photo_abi.cpp (the C ABI) share.
#pragma once
#include "amg.hpp"

namespace fedm {

constexpr int PHOTO_MAX_TERMS = 4;
constexpr int PHOTO_RED_BLOCKS = 256;   // workgroups of a reduction's first pass; the second pass is one workgroup

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
    double *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr;   // CG vectors, nvp each (padding stays 0)
    double *partials = nullptr;   // [2][PHOTO_RED_BLOCKS]
    double *red = nullptr;        // [4] results of a reduction
    int64_t stats[8] = {};        // fedm_photo_stats' order
};
enum PhotoStat { PH_UPDATES = 0, PH_CG_ITS0 = 1, PH_VCYCLES = 5, PH_EXHAUSTED = 6 };

// photo.hip
void launch_photo_load_vector(Ctx &c);   // Photo::g from c.d_uold
void launch_photo_table_write(Ctx &c);   // the targets' c.d_ext from Photo::y
// Conjugate gradients on A x = b from the x it is given, preconditioned by one V-cycle of M (null: Jacobi), until the
// recurrence's residual satisfies |r|_2 <= rtol |b|_2 or max_it steps have run.  Vectors of A.n_rows_p entries whose
// padding is zero; Photo's r, z, p, q are scratch.
struct ScalarCgResult {
    int it;
    double bnorm, rnorm;
};
ScalarCgResult scalar_pcg(Ctx &c, const EllMat &A, Amg *M, const double *b, double *x, double rtol, int max_it);

}  // namespace fedm
