// Conjugate gradients on one scalar vertex system (scalar_cg.hip): the solver of the Helmholtz terms, of the consistent
// field projection and of the weighting potentials.  Each of them owns a ScalarCgWork and hands it to the solve.
#pragma once
#include <cmath>

#include "amg.hpp"

namespace fedm {

constexpr int SCALAR_CG_RED_BLOCKS = 256;   // workgroups of a reduction's first pass; the second pass is one workgroup

struct ScalarCgWork {   // a solve's scratch
    double *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr;   // nvp each (padding stays 0)
    double *partials = nullptr;   // [2][SCALAR_CG_RED_BLOCKS]
    double *red = nullptr;        // [4] results of a reduction
    int alloc(size_t nvp);        // all six, zero-filled, or none (-1): nothing half-made stays behind
    void release();               // (of none or of a released one: nothing happens)
};

struct ScalarCgResult {
    int it;
    double bnorm, rnorm;
    int vcycles;   // the V-cycles of M that ran (Jacobi: 0)
    // 0, FEDM_DIVERGED_NAN (a NaN on the way, or not positive definite) or FEDM_DIVERGED_LINEAR (max_it did not reach rtol)
    int status(double rtol) const {
        if (!std::isfinite(rnorm) || !std::isfinite(bnorm)) return FEDM_DIVERGED_NAN;
        return rnorm > rtol * bnorm ? FEDM_DIVERGED_LINEAR : 0;
    }
};

// Conjugate gradients on A x = b from the x it is given, preconditioned by one V-cycle of M (null: Jacobi), until the
// recurrence's residual satisfies |r|_2 <= rtol |b|_2 or max_it steps have run.  Vectors of A.n_rows_p entries whose
// padding is zero.  Plain launches on the context's stream; every sum has a fixed order.
ScalarCgResult scalar_pcg(Ctx &c, ScalarCgWork &w, const EllMat &A, Amg *M, const double *b, double *x, double rtol,
                          int max_it);

}  // namespace fedm
