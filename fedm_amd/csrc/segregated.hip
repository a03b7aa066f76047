// Kernels of the segregated (uncoupled) time step: fedm_poisson_update and fedm_newton_solve_species (newton.cpp).
//
// The reference solves the potential on its own with the densities frozen (Poisson_solver,
// fedm/functions.py:1154-1161) and then the species among themselves with the field frozen (Source_term with
// coupling='uncoupled', :777-843).  On the device both stages work on ONE matrix, the sliced block-ELL Jacobian of
// the mixed space, and read only the planes of their own diagonal block:
//   * block_product_kernel: y = J_bb x_b for b = the species block or the potential block.  The live planes are a
//     wave-uniform mask (the structurally zero species planes are dropped from it like spmv_kernel's ZMASK drops
//     them), so the species product streams n_s^2 - zeros of the (n_s + 1)^2 planes and the potential product one.
//     The entries of the other block are written as exact zeros: every Krylov vector then has zeros there and the
//     reductions of kernels.hip see the block's entries only.
//   * species_block_inverse_kernel / species_sweep_kernel: the Richardson sweeps z += w_k Duu^-1 (r - J_uu z) of
//     fedm_set_fieldsplit in double precision, the preconditioner of the species systems (one sweep with weight 1:
//     point-block Jacobi).
//   * potential_jacobi_kernel: the potential stage's preconditioner when no multigrid hierarchy is installed.
//   * pick_entries_kernel: a block's entries of a vector, scaled; zeros elsewhere.
#include <hip/hip_runtime.h>

#include "fedm_internal.hpp"
#include "species_planes.hpp"

namespace fedm {

// One wavefront per slice, one lane per vertex (the layout of spmv_kernel).  live: bit r * NEQ + c = plane (r, c) takes
// part.  Rows at or beyond n_owned (padding) are written as zeros.
template <int NEQ>
__global__ __launch_bounds__(256) void block_product_kernel(int n_slices, int n_owned, const int *__restrict__ boff,
                                                            const int *__restrict__ colidx,
                                                            const double *__restrict__ val,
                                                            const double *__restrict__ x, double *__restrict__ y,
                                                            unsigned live) {
    constexpr int NEQ2 = NEQ * NEQ;
    const int slice = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slice >= n_slices) return;
    const int b0 = boff[slice], b1 = boff[slice + 1];
    double acc[NEQ];
#pragma unroll
    for (int r = 0; r < NEQ; ++r) acc[r] = 0.0;
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
                if ((live >> (r * NEQ + cc)) & 1u) acc[r] += vp[(size_t)(r * NEQ + cc) * SLICE] * xj[cc];
    }
    const size_t vtx = (size_t)slice * SLICE + lane;
    const bool owned = (int)vtx < n_owned;
#pragma unroll
    for (int r = 0; r < NEQ; ++r) y[vtx * NEQ + r] = owned ? acc[r] : 0.0;
}

void launch_block_product(Ctx &c, int which, const double *x, double *y) {
    const int n = c.pat.n_slices, neq = c.neq, ns = c.ns;
    if (n == 0) return;
    unsigned live = 0u;
    if (which == 1) {
        live = 1u << (ns * neq + ns);
    } else {
        for (int r = 0; r < ns; ++r)
            for (int cc = 0; cc < ns; ++cc) live |= 1u << (r * neq + cc);
        live &= ~c.zero_plane_mask;
    }
    const dim3 g((n + 3) / 4), b(256);
#define FEDM_BP(NEQ)                                                                                              \
    hipLaunchKernelGGL(block_product_kernel<NEQ>, g, b, 0, c.stream, n, c.n_owned, c.d_slice_boff, c.d_colidx, c.d_val, \
                       x, y, live)
    switch (neq) {
        case 2: FEDM_BP(2); break;
        case 3: FEDM_BP(3); break;
        case 4: FEDM_BP(4); break;
        case 5: FEDM_BP(5); break;
    }
#undef FEDM_BP
}

// Inverse of the n_s x n_s species part of every vertex's diagonal block, sliced: [(slice * NS^2 + e) * 64 + lane]
template <int NS>
__global__ void species_block_inverse_kernel(int nvp, const double *__restrict__ val,
                                             const uint32_t *__restrict__ diag_slot, double *__restrict__ dinv) {
    constexpr int NEQ = NS + 1, NEQ2 = NEQ * NEQ;
    const int vtx = blockIdx.x * blockDim.x + threadIdx.x;
    if (vtx >= nvp) return;
    const uint32_t ds = diag_slot[vtx];
    const double *blk = val + (size_t)(ds >> 6) * NEQ2 * SLICE + (ds & 63);
    double A[NS][NS], I[NS][NS];
#pragma unroll
    for (int r = 0; r < NS; ++r)
#pragma unroll
        for (int cc = 0; cc < NS; ++cc) A[r][cc] = blk[(size_t)(r * NEQ + cc) * SLICE];
    invert_species_block<NS>(A, I);
    const int slice = vtx >> 6, lane = vtx & 63;
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) dinv[((size_t)slice * NS * NS + e) * SLICE + lane] = I[e / NS][e % NS];
}

void launch_species_block_inverse(Ctx &c) {
    const dim3 g((c.nvp + 255) / 256), b(256);
#define FEDM_SBI(NS) \
    hipLaunchKernelGGL(species_block_inverse_kernel<NS>, g, b, 0, c.stream, c.nvp, c.d_val, c.d_diag_slot, c.d_seg_dinv)
    switch (c.ns) {
        case 1: FEDM_SBI(1); break;
        case 2: FEDM_SBI(2); break;
        case 3: FEDM_SBI(3); break;
        case 4: FEDM_SBI(4); break;
    }
#undef FEDM_SBI
}

template <int NS>
__global__ void species_sweep_kernel(int nvp, const double *__restrict__ dinv, double w, const double *__restrict__ r,
                                     const double *__restrict__ t, double *__restrict__ z, int first) {
    constexpr int NEQ = NS + 1;
    const int vtx = blockIdx.x * blockDim.x + threadIdx.x;
    if (vtx >= nvp) return;
    const int slice = vtx >> 6, lane = vtx & 63;
    const double *dp = dinv + (size_t)slice * NS * NS * SLICE + lane;
    double d[NS], z0[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        d[s] = r[(size_t)vtx * NEQ + s] - (first ? 0.0 : t[(size_t)vtx * NEQ + s]);
        z0[s] = first ? 0.0 : z[(size_t)vtx * NEQ + s];
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double a = 0.0;
#pragma unroll
        for (int cc = 0; cc < NS; ++cc) a += dp[(size_t)(s * NS + cc) * SLICE] * d[cc];
        z[(size_t)vtx * NEQ + s] = z0[s] + w * a;
    }
    z[(size_t)vtx * NEQ + NS] = 0.0;
}

void launch_species_sweep(Ctx &c, double w, const double *r, const double *t, double *z, bool first) {
    const dim3 g((c.nvp + 255) / 256), b(256);
#define FEDM_SSW(NS) \
    hipLaunchKernelGGL(species_sweep_kernel<NS>, g, b, 0, c.stream, c.nvp, c.d_seg_dinv, w, r, t, z, first ? 1 : 0)
    switch (c.ns) {
        case 1: FEDM_SSW(1); break;
        case 2: FEDM_SSW(2); break;
        case 3: FEDM_SSW(3); break;
        case 4: FEDM_SSW(4); break;
    }
#undef FEDM_SSW
}

// z_phi = r_phi / (diagonal of the potential-potential plane), z_u = 0: Jacobi for the potential stage without a hierarchy
__global__ void potential_jacobi_kernel(int nvp, int neq, const double *__restrict__ val,
                                        const uint32_t *__restrict__ diag_slot, const double *__restrict__ r,
                                        double *__restrict__ z) {
    const int vtx = blockIdx.x * blockDim.x + threadIdx.x;
    if (vtx >= nvp) return;
    const uint32_t ds = diag_slot[vtx];
    const double a = val[((size_t)(ds >> 6) * neq * neq + (size_t)neq * neq - 1) * SLICE + (ds & 63)];
    for (int s = 0; s < neq - 1; ++s) z[(size_t)vtx * neq + s] = 0.0;
    z[(size_t)vtx * neq + neq - 1] = r[(size_t)vtx * neq + neq - 1] / a;
}

void launch_potential_jacobi(Ctx &c, const double *r, double *z) {
    hipLaunchKernelGGL(potential_jacobi_kernel, dim3((c.nvp + 255) / 256), dim3(256), 0, c.stream, c.nvp, c.neq, c.d_val,
                       c.d_diag_slot, r, z);
}

// (x and y may be the same vector)
__global__ void pick_entries_kernel(size_t n, int neq, int which, double a, const double *x, double *y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool potential = (int)(i % (size_t)neq) == neq - 1;
    y[i] = (potential == (which == 1)) ? a * x[i] : 0.0;
}

void launch_pick_entries(Ctx &c, int which, double a, const double *x, double *y) {
    const size_t n = (size_t)c.np;
    hipLaunchKernelGGL(pick_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, n, c.neq, which, a,
                       x, y);
}

}  // namespace fedm
