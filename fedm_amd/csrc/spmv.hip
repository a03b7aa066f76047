// The matrix side of the Krylov step (gfx950, fp64, HBM-bound): block-Jacobi inverse and row equilibration of the
// diagonal blocks, SpMV on the sliced block-ELL Jacobian (plain, with the first field-split stage, and fused with the
// step's dot products and their finish), and y = alpha Dinv x.
#include <cstdlib>
#include <type_traits>

#include "device_util.hpp"
#include "fedm_internal.hpp"

namespace fedm {

// =============================================================================================
// Point-block Jacobi: inverse of every vertex's n_eq x n_eq diagonal block (Gauss-Jordan with
// partial pivoting), stored sliced so that lanes are contiguous.
// =============================================================================================
template <int NEQ>
__global__ void block_inverse_kernel(int nvp, const double *__restrict__ val,
                                     const uint32_t *__restrict__ diag_slot,
                                     double *__restrict__ dinv) {
    constexpr int NEQ2 = NEQ * NEQ;
    const int vtx = blockIdx.x * blockDim.x + threadIdx.x;
    if (vtx >= nvp) return;
    const uint32_t ds = diag_slot[vtx];
    double A[NEQ][NEQ], I[NEQ][NEQ];
#pragma unroll
    for (int r = 0; r < NEQ; ++r)
#pragma unroll
        for (int cidx = 0; cidx < NEQ; ++cidx) {
            A[r][cidx] = val[((size_t)(ds >> 6) * NEQ2 + r * NEQ + cidx) * SLICE + (ds & 63)];
            I[r][cidx] = (r == cidx) ? 1.0 : 0.0;
        }
#pragma unroll
    for (int k = 0; k < NEQ; ++k) {
        // partial pivoting without dynamic register indexing: swap rows by predication
        int piv = k;
        double best = fabs(A[k][k]);
#pragma unroll
        for (int r = k + 1; r < NEQ; ++r)
            if (fabs(A[r][k]) > best) {
                best = fabs(A[r][k]);
                piv = r;
            }
#pragma unroll
        for (int r = k + 1; r < NEQ; ++r)
            if (piv == r) {
#pragma unroll
                for (int cidx = 0; cidx < NEQ; ++cidx) {
                    double t = A[k][cidx];
                    A[k][cidx] = A[r][cidx];
                    A[r][cidx] = t;
                    t = I[k][cidx];
                    I[k][cidx] = I[r][cidx];
                    I[r][cidx] = t;
                }
            }
        const double inv = 1.0 / A[k][k];
#pragma unroll
        for (int cidx = 0; cidx < NEQ; ++cidx) {
            A[k][cidx] *= inv;
            I[k][cidx] *= inv;
        }
#pragma unroll
        for (int r = 0; r < NEQ; ++r) {
            if (r == k) continue;
            const double f = A[r][k];
#pragma unroll
            for (int cidx = 0; cidx < NEQ; ++cidx) {
                A[r][cidx] -= f * A[k][cidx];
                I[r][cidx] -= f * I[k][cidx];
            }
        }
    }
    const int slice = vtx >> 6, lane = vtx & 63;
#pragma unroll
    for (int e = 0; e < NEQ2; ++e) dinv[((size_t)slice * NEQ2 + e) * SLICE + lane] = I[e / NEQ][e % NEQ];
}

void launch_block_inverse(Ctx &c) {
    const dim3 g((c.nvp + 255) / 256), b(256);
    switch (c.neq) {
        case 1: hipLaunchKernelGGL(block_inverse_kernel<1>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, c.d_dinv); break;
        case 2: hipLaunchKernelGGL(block_inverse_kernel<2>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, c.d_dinv); break;
        case 3: hipLaunchKernelGGL(block_inverse_kernel<3>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, c.d_dinv); break;
        case 4: hipLaunchKernelGGL(block_inverse_kernel<4>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, c.d_dinv); break;
        case 5: hipLaunchKernelGGL(block_inverse_kernel<5>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, c.d_dinv); break;
        case 6: hipLaunchKernelGGL(block_inverse_kernel<6>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, c.d_dinv); break;
    }
}

// Row equilibration of the Krylov residual test (fedm_set_krylov_scaling): for the DOF (vertex v, component r)
// s = sqrt(sum_c J[(v,r),(v,c)]^2) over row r of the vertex's diagonal block, d = 1 / s (1 where s is zero or not
// finite: identity rows get exactly 1).  A thread per vertex, the planes block_inverse_kernel reads; d2 = d^2 is what
// the weighted reductions multiply by, d itself is written only for whoever asks (fedm_get_krylov_scaling).
template <int NEQ>
__global__ void row_scale_kernel(int nvp, const double *__restrict__ val, const uint32_t *__restrict__ diag_slot,
                                 double *__restrict__ d2, double *__restrict__ d_out) {
    constexpr int NEQ2 = NEQ * NEQ;
    const int vtx = blockIdx.x * blockDim.x + threadIdx.x;
    if (vtx >= nvp) return;
    const uint32_t ds = diag_slot[vtx];
    const double *blk = val + (size_t)(ds >> 6) * NEQ2 * SLICE + (ds & 63);
#pragma unroll
    for (int r = 0; r < NEQ; ++r) {
        double s2 = 0.0;
#pragma unroll
        for (int cidx = 0; cidx < NEQ; ++cidx) {
            const double a = blk[(size_t)(r * NEQ + cidx) * SLICE];
            s2 += a * a;
        }
        const double s = sqrt(s2);
        const double d = (s > 0.0 && s < 1.7e308) ? 1.0 / s : 1.0;   // (NaN fails both comparisons)
        d2[(size_t)vtx * NEQ + r] = d * d;
        if (d_out) d_out[(size_t)vtx * NEQ + r] = d;
    }
}

void launch_row_scale(Ctx &c, double *d2, double *d_out) {
    const dim3 g((c.nvp + 255) / 256), b(256);
    switch (c.neq) {
        case 1: hipLaunchKernelGGL(row_scale_kernel<1>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, d2, d_out); break;
        case 2: hipLaunchKernelGGL(row_scale_kernel<2>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, d2, d_out); break;
        case 3: hipLaunchKernelGGL(row_scale_kernel<3>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, d2, d_out); break;
        case 4: hipLaunchKernelGGL(row_scale_kernel<4>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, d2, d_out); break;
        case 5: hipLaunchKernelGGL(row_scale_kernel<5>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, d2, d_out); break;
        case 6: hipLaunchKernelGGL(row_scale_kernel<6>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, d2, d_out); break;
    }
}

// =============================================================================================
// SpMV on the sliced block-ELL matrix: one wavefront per slice, one lane per vertex.
// Matrix values and column indices stream in coalesced (lanes contiguous); x is gathered per
// neighbour (n_eq contiguous doubles).  Optional fused block-Jacobi scaling y = Dinv (A x).
// =============================================================================================
// ZMASK: bit (r * NEQ + c) marks a value plane that is structurally zero for this model (no reaction
// couples the two species: d(electron row)/d(ion density) of the streamer model) -- it is neither
// loaded nor multiplied: one ninth of the streamer matrix's bytes.
template <int NEQ, bool FS, unsigned ZMASK = 0u>
__global__ __launch_bounds__(256) void spmv_kernel(int n_slices, int n_owned,
                                                   const int *__restrict__ boff,
                                                   const int *__restrict__ colidx,
                                                   const double *__restrict__ val,
                                                   const double *__restrict__ x,
                                                   double *__restrict__ y,
                                                   const double *__restrict__ dinv,
                                                   double *__restrict__ fs_z, double *__restrict__ fs_b0,
                                                   double fs_scale, const int *__restrict__ slice_list,
                                                   int fs_compact32 = 0, int xcd = 0) {
    constexpr int NEQ2 = NEQ * NEQ;
    // xcd: consecutive slices (neighbours in the Z-curve, sharing most of their x entries) on one XCD
    const int blk = (xcd & 1) ? xcd_contiguous(blockIdx.x, gridDim.x) : blockIdx.x;
    const int wave_id = blk * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (wave_id >= n_slices) return;  // n_slices: number of slices this launch covers
    const int slice = slice_list ? slice_list[wave_id] : wave_id;
    const int b0 = boff[slice], b1 = boff[slice + 1];
    // epilogue operands (block inverse) requested before the gather loop
    constexpr int ND = FS ? (NEQ - 1) * (NEQ - 1) : NEQ2;
    double dv[ND > 0 ? ND : 1];
    if (FS || dinv) {
        const double *dp = dinv + (size_t)slice * ND * SLICE + lane;
#pragma unroll
        for (int e = 0; e < ND; ++e) dv[e] = dp[(size_t)e * SLICE];
    }
    double acc[NEQ];
#pragma unroll
    for (int r = 0; r < NEQ; ++r) acc[r] = 0.0;
    // xcd bit 1: the matrix values by non-temporal loads (launch_spmv: matrices beyond half the Infinity Cache).  Read
    // once per product, they then neither go through the cache nor push the vectors, the preconditioner's planes and
    // the multigrid out of it: the 4 M-DOF product 136 -> 123 us (69 -> 76 % of the HBM peak), the 1 M-DOF time step
    // -2.7 % and the developed streamer's -3.6 % although the product by itself, back to back, slows from 28 to 35 us
    // there (its 177 MB would have stayed in the cache if nothing else ran).
    auto products = [&](auto nt_c) {
        constexpr bool NT = decltype(nt_c)::value;
        for (int bc = b0; bc < b1; ++bc) {
            const int col = colidx[(size_t)bc * SLICE + lane];
            double xj[NEQ];
#pragma unroll
            for (int cc = 0; cc < NEQ; ++cc) xj[cc] = x[(size_t)col * NEQ + cc];
            const double *vp = val + (size_t)bc * NEQ2 * SLICE + lane;
#pragma unroll
            for (int r = 0; r < NEQ; ++r)
#pragma unroll
                for (int cc = 0; cc < NEQ; ++cc)
                    if (!((ZMASK >> (r * NEQ + cc)) & 1u)) {
                        const double *ap = &vp[(size_t)(r * NEQ + cc) * SLICE];
                        acc[r] += (NT ? __builtin_nontemporal_load(ap) : *ap) * xj[cc];
                    }
        }
    };
    if (xcd & 2) products(std::true_type{});
    else products(std::false_type{});
    const size_t vtx = (size_t)slice * SLICE + lane;
    if ((int)vtx >= n_owned) {  // ghost / padding rows belong to someone else (or to nobody)
#pragma unroll
        for (int r = 0; r < NEQ; ++r) acc[r] = 0.0;
    }
    if (FS) {
        // first stage of the field-split preconditioner in the epilogue (amg.hip):
        // t = A x is kept, z_u = fs_scale * Duu^-1 t_u starts the species sweeps, b0 = t_phi
        constexpr int NS = NEQ - 1;
#pragma unroll
        for (int r = 0; r < NEQ; ++r) y[vtx * NEQ + r] = acc[r];
#pragma unroll
        for (int r = 0; r < NS; ++r) {
            double z = 0.0;
#pragma unroll
            for (int cc = 0; cc < NS; ++cc) z += dv[r * NS + cc] * acc[cc];
            // (with sweeps to follow the first species iterate is a compact single-precision vector)
            if (fs_compact32) reinterpret_cast<float *>(fs_z)[vtx * NS + r] = (float)(fs_scale * z);
            else fs_z[vtx * NEQ + r] = fs_scale * z;
        }
        if (!fs_compact32) fs_z[vtx * NEQ + NS] = 0.0;  // whole lines are written; the V-cycle result lands here later
        fs_b0[vtx] = acc[NS];
    } else if (dinv) {
#pragma unroll
        for (int r = 0; r < NEQ; ++r) {
            double z = 0.0;
#pragma unroll
            for (int cc = 0; cc < NEQ; ++cc) z += dv[r * NEQ + cc] * acc[cc];
            y[vtx * NEQ + r] = z;
        }
    } else {
#pragma unroll
        for (int r = 0; r < NEQ; ++r) y[vtx * NEQ + r] = acc[r];
    }
}

// bit 1 of the products' `xcd` argument: the Jacobian's values by non-temporal loads when the matrix is larger than half
// the Infinity Cache (256 MiB) -- see spmv_kernel; FEDM_SPMV_NT=0 / 1 forces it off / on
static int spmv_nontemporal(const Ctx &c) {
    static const int forced = [] {
        const char *e = std::getenv("FEDM_SPMV_NT");
        return e ? (e[0] == '0' ? 0 : 1) : -1;
    }();
    if (forced >= 0) return forced ? 2 : 0;
    const double bytes = (double)c.pat.total_bc * SLICE * c.neq * c.neq * sizeof(double);
    return bytes > 128.0 * 1024.0 * 1024.0 ? 2 : 0;
}

// slice_list != nullptr: only those n_list matrix slices (interior / boundary halves across GPUs)
void launch_spmv(Ctx &c, const double *x, double *y, bool scale_dinv, const int *slice_list, int n_list) {
    const int n = slice_list ? n_list : c.pat.n_slices;
    if (n == 0) return;
    const dim3 g((n + 3) / 4), b(256);
    const double *dinv = scale_dinv ? c.d_dinv : nullptr;
#define FEDM_SPMV_Z(NEQ, Z)                                                                           \
    hipLaunchKernelGGL((spmv_kernel<NEQ, false, Z>), g, b, 0, c.stream, n, c.n_owned, c.d_slice_boff, \
                       c.d_colidx, c.d_val, x, y, dinv, (double *)nullptr, (double *)nullptr, 0.0,         \
                       slice_list, 0, ((c.xcd_remap && !slice_list) ? 1 : 0) | spmv_nontemporal(c))
#define FEDM_SPMV(NEQ) FEDM_SPMV_Z(NEQ, 0u)
    switch (c.neq) {
        case 1: FEDM_SPMV(1); break;
        case 2: FEDM_SPMV(2); break;
        case 3:  // two species + potential: the species-species planes (0,1) / (1,0) may be zero
            switch (c.zero_plane_mask & 10u) {
                case 2u: FEDM_SPMV_Z(3, 2u); break;
                case 8u: FEDM_SPMV_Z(3, 8u); break;
                case 10u: FEDM_SPMV_Z(3, 10u); break;
                default: FEDM_SPMV(3); break;
            }
            break;
        case 4: FEDM_SPMV(4); break;
        case 5: FEDM_SPMV(5); break;
        case 6: FEDM_SPMV(6); break;
    }
#undef FEDM_SPMV
#undef FEDM_SPMV_Z
}

// t = A x together with the first field-split stage (c.d_dinv holds the species-block inverses);
// slice_list != nullptr: only those n_list matrix slices (interior / boundary halves across GPUs)
void launch_spmv_fieldsplit(Ctx &c, const double *x, double *t, double *z, double *b0, double scale,
                            const int *slice_list, int n_list, bool compact32) {
    const int n = slice_list ? n_list : c.pat.n_slices;
    if (n == 0) return;
    const dim3 g((n + 3) / 4), b(256);
#define FEDM_SPMV_Z(NEQ, Z)                                                                          \
    hipLaunchKernelGGL((spmv_kernel<NEQ, true, Z>), g, b, 0, c.stream, n, c.n_owned, c.d_slice_boff, \
                       c.d_colidx, c.d_val, x, t, c.d_dinv, z, b0, scale, slice_list, compact32 ? 1 : 0,      \
                       ((c.xcd_remap && !slice_list) ? 1 : 0) | spmv_nontemporal(c))
#define FEDM_SPMV(NEQ) FEDM_SPMV_Z(NEQ, 0u)
    switch (c.neq) {
        case 2: FEDM_SPMV(2); break;
        case 3:
            switch (c.zero_plane_mask & 10u) {
                case 2u: FEDM_SPMV_Z(3, 2u); break;
                case 8u: FEDM_SPMV_Z(3, 8u); break;
                case 10u: FEDM_SPMV_Z(3, 10u); break;
                default: FEDM_SPMV(3); break;
            }
            break;
        case 4: FEDM_SPMV(4); break;
        case 5: FEDM_SPMV(5); break;
        case 6: FEDM_SPMV(6); break;
    }
#undef FEDM_SPMV
#undef FEDM_SPMV_Z
}

// y = alpha * Dinv x
template <int NEQ>
__global__ void apply_dinv_kernel(int nvp, const double *__restrict__ dinv,
                                  const double *__restrict__ x, double *__restrict__ y, double alpha) {
    constexpr int NEQ2 = NEQ * NEQ;
    const int vtx = blockIdx.x * blockDim.x + threadIdx.x;
    if (vtx >= nvp) return;
    const int slice = vtx >> 6, lane = vtx & 63;
    const double *dp = dinv + (size_t)slice * NEQ2 * SLICE + lane;
    double xv[NEQ];
#pragma unroll
    for (int cc = 0; cc < NEQ; ++cc) xv[cc] = x[(size_t)vtx * NEQ + cc];
#pragma unroll
    for (int r = 0; r < NEQ; ++r) {
        double z = 0.0;
#pragma unroll
        for (int cc = 0; cc < NEQ; ++cc) z += dp[(size_t)(r * NEQ + cc) * SLICE] * xv[cc];
        y[(size_t)vtx * NEQ + r] = alpha * z;
    }
}

void launch_apply_dinv(Ctx &c, const double *x, double *y, double alpha) {
    const dim3 g((c.nvp + 255) / 256), b(256);
    switch (c.neq) {
        case 1: hipLaunchKernelGGL(apply_dinv_kernel<1>, g, b, 0, c.stream, c.nvp, c.d_dinv, x, y, alpha); break;
        case 2: hipLaunchKernelGGL(apply_dinv_kernel<2>, g, b, 0, c.stream, c.nvp, c.d_dinv, x, y, alpha); break;
        case 3: hipLaunchKernelGGL(apply_dinv_kernel<3>, g, b, 0, c.stream, c.nvp, c.d_dinv, x, y, alpha); break;
        case 4: hipLaunchKernelGGL(apply_dinv_kernel<4>, g, b, 0, c.stream, c.nvp, c.d_dinv, x, y, alpha); break;
        case 5: hipLaunchKernelGGL(apply_dinv_kernel<5>, g, b, 0, c.stream, c.nvp, c.d_dinv, x, y, alpha); break;
        case 6: hipLaunchKernelGGL(apply_dinv_kernel<6>, g, b, 0, c.stream, c.nvp, c.d_dinv, x, y, alpha); break;
    }
}

// Krylov steps with at most eight reduction slots (the first seven steps of a solve: all there are early in a
// streamer run, most of them later): the Jacobian product w = J z and the step's dot products v_i . w, w . w in ONE kernel -- the wave
// that has formed a slice's rows of w multiplies them with the same rows of the basis vectors before it stores them
// (w is not read back: 8 MB and a 9 us kernel less per step).  One partial per workgroup and slot,
// partials[slot * n_blocks + block]; spmv_dots_finish_kernel reduces them in a fixed order.
// W: the dot products in the weighted inner product (dots_kernel); the rows' weights are read once the rows are formed.
template <int NEQ, unsigned ZMASK, int K, bool W = false>
__global__ __launch_bounds__(256) void spmv_dots_kernel(int n_slices, int n_owned, const int *__restrict__ boff,
                                                        const int *__restrict__ colidx,
                                                        const double *__restrict__ val,
                                                        const double *__restrict__ x, double *__restrict__ y,
                                                        PtrPack8 xs, double *__restrict__ partials, int xcd,
                                                        const double *__restrict__ wgt = nullptr) {
    constexpr int NEQ2 = NEQ * NEQ;
    const int blk = (xcd & 1) ? xcd_contiguous(blockIdx.x, gridDim.x) : blockIdx.x;
    const int wave_id = blk * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool live = wave_id < n_slices;          // (no early return: the workgroup reduces together)
    const int slice = live ? wave_id : 0;
    const int b0 = boff[slice], b1 = live ? boff[slice + 1] : b0;
    double acc[NEQ];
#pragma unroll
    for (int r = 0; r < NEQ; ++r) acc[r] = 0.0;
    // xcd bit 1: the matrix values by non-temporal loads (launch_spmv: matrices beyond half the Infinity Cache).  Read
    // once per product, they then neither go through the cache nor push the vectors, the preconditioner's planes and
    // the multigrid out of it: the 4 M-DOF product 136 -> 123 us (69 -> 76 % of the HBM peak), the 1 M-DOF time step
    // -2.7 % and the developed streamer's -3.6 % although the product by itself, back to back, slows from 28 to 35 us
    // there (its 177 MB would have stayed in the cache if nothing else ran).
    auto products = [&](auto nt_c) {
        constexpr bool NT = decltype(nt_c)::value;
        for (int bc = b0; bc < b1; ++bc) {
            const int col = colidx[(size_t)bc * SLICE + lane];
            double xj[NEQ];
#pragma unroll
            for (int cc = 0; cc < NEQ; ++cc) xj[cc] = x[(size_t)col * NEQ + cc];
            const double *vp = val + (size_t)bc * NEQ2 * SLICE + lane;
#pragma unroll
            for (int r = 0; r < NEQ; ++r)
#pragma unroll
                for (int cc = 0; cc < NEQ; ++cc)
                    if (!((ZMASK >> (r * NEQ + cc)) & 1u)) {
                        const double *ap = &vp[(size_t)(r * NEQ + cc) * SLICE];
                        acc[r] += (NT ? __builtin_nontemporal_load(ap) : *ap) * xj[cc];
                    }
        }
    };
    if (xcd & 2) products(std::true_type{});
    else products(std::false_type{});
    const size_t vtx = (size_t)slice * SLICE + lane;
    const bool owned = live && (int)vtx < n_owned;
    double d[K];
#pragma unroll
    for (int i = 0; i < K; ++i) d[i] = 0.0;
    if constexpr (W) {
        // the rows are stored first and then weighted in place: no registers beyond the unweighted kernel's
        if (live) {
#pragma unroll
            for (int r = 0; r < NEQ; ++r) y[vtx * NEQ + r] = owned ? acc[r] : 0.0;
        }
        if (owned) {
#pragma unroll
            for (int r = 0; r < NEQ; ++r) {
                const double a = acc[r];
                acc[r] = a * wgt[vtx * NEQ + r];
                d[K - 1] += a * acc[r];
            }
            // (the weights' registers are free before the basis vectors' loads are issued: without this the scheduler
            // hoists those loads above the scaling and the K = 7 instantiation loses a wave per SIMD)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < K - 1; ++i)
#pragma unroll
                for (int r = 0; r < NEQ; ++r) d[i] += xs.p[i][vtx * NEQ + r] * acc[r];
        }
    } else {
        if (owned) {
#pragma unroll
            for (int i = 0; i < K - 1; ++i)
#pragma unroll
                for (int r = 0; r < NEQ; ++r) d[i] += xs.p[i][vtx * NEQ + r] * acc[r];
#pragma unroll
            for (int r = 0; r < NEQ; ++r) d[K - 1] += acc[r] * acc[r];
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < NEQ; ++r) y[vtx * NEQ + r] = owned ? acc[r] : 0.0;
        }
    }
    __shared__ double sm[4][K];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double t = wave_sum(d[i]);
        if (lane == 0) sm[wave][i] = t;
    }
    __syncthreads();
    if (threadIdx.x < K)
        partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] =
            sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] + sm[3][threadIdx.x];
}

// reduce_finish_kernel for the partials of spmv_dots_kernel (one per workgroup of the product: thousands, not
// RED_BLOCKS): the 16 waves share the k <= 8 slots, wave w sums the blocks of chunk w / k of slot w % k, the chunks
// are added in their order; then the formulae and the publication of cgs_finish_kernel.
// finish: 0 the local sums only, 1 formulae and publication, 2 (a refined step, krylov.cpp) the formulae and the flag
// out[RED_REFINE] = 1 when the cancellation was too strong, without a publication.
__global__ __launch_bounds__(1024) void spmv_dots_finish_kernel(const double *__restrict__ partials, int nblocks,
                                                               int k, double *__restrict__ out, double *mail,
                                                               unsigned long long *seq, int finish) {
    __shared__ double fin[RED_K];
    __shared__ double part[16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < RED_K) fin[threadIdx.x] = (threadIdx.x == RED_SPARE) ? out[RED_SPARE] : 0.0;
    const int chunks = 16 / k, slot = wave % k, chunk = wave / k;
    double sum = 0.0;
    if (chunk < chunks)
        for (int b = chunk * 64 + lane; b < nblocks; b += chunks * 64) sum += partials[(size_t)slot * nblocks + b];
    sum = wave_sum(sum);
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x < k) {
        double t = 0.0;
        for (int ch = 0; ch < chunks; ++ch) t += part[ch * k + threadIdx.x];
        fin[threadIdx.x] = t;
        if (!finish) out[threadIdx.x] = t;   // several GPUs: the local sums, for the all-reduce that follows
    }
    if (!finish) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double ww = fin[k - 1];
        double hh = 0.0;
        for (int i = 0; i < k - 1; ++i) hh += fin[i] * fin[i];
        const double hn2 = ww - hh;
        fin[RED_K - 2] = ww;
        fin[k - 1] = hn2;
        const bool sound = hn2 > 1e-8 * ww && hn2 > 0.0;
        fin[RED_K - 1] = sound ? 1.0 / sqrt(hn2) : 1.0;
        if (finish == 2) fin[RED_REFINE] = sound ? 0.0 : 1.0;   // what the second pass behind this step reads
    }
    __syncthreads();
    if (finish == 2) {   // a refined step: its one publication is refine_finish_kernel's
        if (threadIdx.x < RED_K) out[threadIdx.x] = fin[threadIdx.x];
        return;
    }
    if (threadIdx.x < 64) {
        const unsigned long long tag = *seq + 1;
        double *slot_ = mail + (tag & (MAIL_SLOTS - 1)) * (RED_K + 1);
        for (int i = threadIdx.x; i < RED_K; i += 64) {
            out[i] = fin[i];
            slot_[i] = fin[i];
        }
        __threadfence_system();
        if (threadIdx.x == 0) {
            *seq = tag;
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(slot_ + RED_K), tag, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// w = J z with the step's k = j + 2 reduction slots (xs[0 .. k-2] . w and w . w), finished and published: one GPU,
// three species-plus-potential equations, k <= 8, buffers of ensure_spmv_dots.  false: not applicable (nothing was
// launched; the caller runs launch_spmv + launch_dots_fused).
bool spmv_dots_applicable(const Ctx &c, int k) {
    static const bool off = [] {
        const char *e = std::getenv("FEDM_SPMV_DOTS");
        return e && e[0] == '0';
    }();
    // (several GPUs: where the whole product is one launch -- deep halos -- with finish = false)
    return !off && c.neq == 3 && k >= 2 && k <= 8 && c.d_partials_wide;
}

bool launch_spmv_dots(Ctx &c, const double *x, double *y, const double *const *xs, int k, int finish) {
    if (!spmv_dots_applicable(c, k)) return false;
    const int n = c.pat.n_slices;
    const dim3 g((n + 3) / 4), b(256);
    PtrPack8 pk;
    for (int i = 0; i < 8; ++i) pk.p[i] = xs[i < k - 1 ? i : 0];
    const int xcd = (c.xcd_remap ? 1 : 0) | spmv_nontemporal(c);
#define FEDM_SD(Z, K)                                                                                       \
    if (c.red_w) hipLaunchKernelGGL((spmv_dots_kernel<3, Z, K, true>), g, b, 0, c.stream, n, c.n_owned,       \
                                    c.d_slice_boff, c.d_colidx, c.d_val, x, y, pk, c.d_partials_wide, xcd, c.red_w); \
    else hipLaunchKernelGGL((spmv_dots_kernel<3, Z, K>), g, b, 0, c.stream, n, c.n_owned, c.d_slice_boff, c.d_colidx, \
                            c.d_val, x, y, pk, c.d_partials_wide, xcd)
#define FEDM_SD_K(Z)                                                                                        \
    do {                                                                                                    \
        if (k == 2) FEDM_SD(Z, 2);                                                                          \
        else if (k == 3) FEDM_SD(Z, 3);                                                                     \
        else if (k == 4) FEDM_SD(Z, 4);                                                                     \
        else if (k == 5) FEDM_SD(Z, 5);                                                                     \
        else if (k == 6) FEDM_SD(Z, 6);                                                                     \
        else if (k == 7) FEDM_SD(Z, 7);                                                                     \
        else FEDM_SD(Z, 8);                                                                                 \
    } while (0)
    switch (c.zero_plane_mask & 10u) {
        case 2u: FEDM_SD_K(2u); break;
        case 8u: FEDM_SD_K(8u); break;
        case 10u: FEDM_SD_K(10u); break;
        default: FEDM_SD_K(0u); break;
    }
#undef FEDM_SD_K
#undef FEDM_SD
    hipLaunchKernelGGL(spmv_dots_finish_kernel, dim3(1), dim3(1024), 0, c.stream, c.d_partials_wide, (int)g.x, k,
                       c.d_red, c.h_mail, c.d_mail_seq, finish);
    if (finish == SPMV_DOTS_PUBLISH && !c.capturing) ++c.mail_seq;
    return true;
}

// (one partial per workgroup of the product and slot; allocated with the Krylov vectors, outside any capture)
int ensure_spmv_dots(Ctx &c) {
    if (c.d_partials_wide || c.neq != 3) return 0;
    const size_t blocks = (size_t)(c.pat.n_slices + 3) / 4;
    FEDM_HIP_CHECK(hipMalloc((void **)&c.d_partials_wide, sizeof(double) * 8 * blocks));
    return 0;
}

}  // namespace fedm
