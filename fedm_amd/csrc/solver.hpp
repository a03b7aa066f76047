// Declarations shared by the translation units of the C ABI (context.cpp, krylov.cpp, newton.cpp, amg_setup.cpp,
// hooks.cpp).  Host code only: what the kernels' sources share is in fedm_internal.hpp.
#pragma once
#include "amg.hpp"
#include "comm.hpp"
#include "fedm_internal.hpp"

struct fedm_ctx {
    fedm::Ctx c;
};

namespace fedm {

// context.cpp: a host vector of c.n entries to / from a device vector, through the pinned staging buffer
int put_vec(Ctx &c, double *dst, const double *src);
int get_vec(Ctx &c, double *dst, const double *src);

// krylov.cpp
int ensure_krylov(Ctx &c, int restart);
bool right_preconditioned(const Ctx &c);
void prepare_preconditioner_and_rhs(Ctx &c);
void krylov_vector_update(Ctx &c, int k, const double *const *vp, double *w);
void krylov_vector_scale(Ctx &c, double a, const double *x, double *y);
int gmres(Ctx &c, int restart, double rtol, double atol, int max_it, int *its_out, double *rnorm_out,
          const double *bvec, double bscale, double bnorm_known, double *u_update, bool *u_updated,
          int newton_iteration = -1);   // which solve of a Newton loop this is (-1: none): the hint slot it reads and writes
int species_gmres(Ctx &c, int restart, double rtol, double atol, int max_it, double bnorm, int *its_out,
                  double *rnorm_out);
// Preconditioned CG on the potential rows: the residual in c.d_rhs, the accumulated correction left in c.d_V
// (ensure_krylov(c, 1) first); c.d_tmp, c.d_delta and c.d_w are scratch.
enum class CgMatrix { whole, potential_block };   // the product and the preconditioner used without a hierarchy
struct CgResult {
    int it;
    double r0, rn;   // |r| before the first and after the last iteration
};
CgResult preconditioned_cg(Ctx &c, CgMatrix matrix, double rtol, int max_it);

// amg_setup.cpp: a hierarchy of n_first_rows unknowns built and uploaded into *out (the potential block's, the
// replicated global one, a photoionisation term's).  composite_from: the first level that may fold its smoother into
// composite operators (beyond the last level: plain sweeps everywhere).
int build_amg(Ctx &c, int n_first_rows, int n_levels, const fedm_csr *A, const fedm_csr *P, const fedm_csr *R,
              const double *coarse_inverse, int nu, double omega, Amg **out, int composite_from,
              const double *poly_w = nullptr /* [n_levels - 1][nu] */);

// newton.cpp
void set_hard_mode(Ctx &c, bool hard);
int segregated_refusal(Ctx &c, const char *who, bool species);
int ensure_seg_dinv(Ctx &c);
enum SegStat { SG_UPDATES = 0, SG_CG_ITS, SG_SOLVES, SG_ONE_PASS, SG_FALLBACK, SG_NEWTON_ITS, SG_KRYLOV_STEPS };

}  // namespace fedm
