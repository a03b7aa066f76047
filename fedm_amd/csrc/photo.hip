// Photoionisation in the three-term Helmholtz approximation (include/fedm_hip.h, fedm_photo_setup): the load vector
// of the ionisation rate at u_old, conjugate gradients on the terms' operators, and the source tables the element
// routines read.  Plain launches on the context's stream; no kernel waits for another workgroup and none adds with
// atomics: every sum has a fixed order, so an update is bitwise reproducible.
#include "photo.hpp"

#include <algorithm>
#include <cmath>

#include "device_util.hpp"
#include "element.hpp"

namespace fedm {

// ---- load vector -------------------------------------------------------------------------------
struct PhotoSources {
    int n_src;
    int src[FEDM_MAX_REACTIONS];
    double efficiency;
};

// A thread per cell: g_loc[a] = sum_q w_q |det J| w(x_q) efficiency R(x_q) phi_a(x_q), R = sum_j k_j(|E|) prod_i n_i^P_ji
// with |E| and the k_j once per cell, as Element::setup has them (P1: grad(Phi) is constant on the cell), and the
// densities at the model's quadrature points.  w = r for an axisymmetric model, 1 otherwise.
template <int NS, bool PO, bool TAB>
__global__ __launch_bounds__(256) void photo_cell_load_kernel(int nc, const fedm_model_desc *__restrict__ md,
                                                              const double *__restrict__ coords,
                                                              const int *__restrict__ cells,
                                                              const double *__restrict__ u, PhotoSources ps,
                                                              double *__restrict__ cell_g) {
    constexpr int NEQ = NS + (PO ? 1 : 0);
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= nc) return;
    double x[3][2], U[3][NEQ];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int v = cells[3 * cell + a];
        x[a][0] = coords[2 * (size_t)v];
        x[a][1] = coords[2 * (size_t)v + 1];
#pragma unroll
        for (int e = 0; e < NEQ; ++e) U[a][e] = u[(size_t)v * NEQ + e];
    }
    const bool axi = md->axisymmetric != 0, lin = md->linear_representation != 0;
    CellGeom cg;
    cg.init(x, axi);
    double Em = 1.0, invEm = 1.0;
    if (PO) {
        double gx = 0.0, gy = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            gx += U[a][NEQ - 1] * cg.G[a][0];
            gy += U[a][NEQ - 1] * cg.G[a][1];
        }
        Em = sqrt(gx * gx + gy * gy);
        invEm = 1.0 / Em;
    }
    const double lnE = log(Em);
    double wn[3], acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 3; ++a) wn[a] = axi ? x[a][0] : 1.0;
    const int nq = md->n_qp;
    for (int k = 0; k < ps.n_src; ++k) {
        const int j = ps.src[k];
        double kv, kd;
        termsum_eval<TAB>(md, md->k[j], Em, invEm, lnE, kv, kd);
        for (int q = 0; q < nq; ++q) {
            const double xq = md->qp_x[q], yq = md->qp_y[q];
            const double phi[3] = {1.0 - xq - yq, xq, yq};
            double prod = 1.0;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int P = md->power[j][i];
                if (!P) continue;
                const double ui = U[0][i] * phi[0] + U[1][i] * phi[1] + U[2][i] * phi[2];
                const double n = lin ? ui : exp(ui);
                for (int e = 0; e < P; ++e) prod *= n;
            }
            const double W = md->qp_w[q] * cg.detJ * (wn[0] * phi[0] + wn[1] * phi[1] + wn[2] * phi[2]);
            const double f = W * ps.efficiency * kv * prod;
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[a] += f * phi[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) cell_g[3 * (size_t)cell + a] = acc[a];
}

// A thread per vertex: its cells' entries in the order of the list (ascending cell, then corner); 0 on the zero
// vertices and the padding.
__global__ __launch_bounds__(256) void photo_vertex_sum_kernel(int nv, int nvp, const int *__restrict__ v_ptr,
                                                               const int *__restrict__ v_idx,
                                                               const unsigned char *__restrict__ zero,
                                                               const double *__restrict__ cell_g,
                                                               double *__restrict__ g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvp) return;
    double s = 0.0;
    if (v < nv && !zero[v])
        for (int k = v_ptr[v]; k < v_ptr[v + 1]; ++k) s += cell_g[v_idx[k]];
    g[v] = s;
}

void launch_photo_load_vector(Ctx &c) {
    Photo &ph = *c.photo;
    PhotoSources ps{};
    ps.n_src = ph.desc.n_src;
    for (int k = 0; k < ps.n_src; ++k) ps.src[k] = ph.desc.src_reaction[k];
    ps.efficiency = ph.desc.efficiency;
    const dim3 gc((c.nc + 255) / 256), gv((c.nvp + 255) / 256), b(256);
#define FEDM_PHOTO_LOAD(NS_, PO_)                                                                                  \
    do {                                                                                                           \
        if (c.model_tables)                                                                                        \
            hipLaunchKernelGGL((photo_cell_load_kernel<NS_, PO_, true>), gc, b, 0, c.stream, c.nc, c.d_model,      \
                               c.d_coords, c.d_cells, c.d_uold, ps, ph.cell_g);                                    \
        else                                                                                                       \
            hipLaunchKernelGGL((photo_cell_load_kernel<NS_, PO_, false>), gc, b, 0, c.stream, c.nc, c.d_model,     \
                               c.d_coords, c.d_cells, c.d_uold, ps, ph.cell_g);                                    \
    } while (0)
    if (c.poisson) {
        switch (c.ns) {
            case 1: FEDM_PHOTO_LOAD(1, true); break;
            case 2: FEDM_PHOTO_LOAD(2, true); break;
            case 3: FEDM_PHOTO_LOAD(3, true); break;
            default: FEDM_PHOTO_LOAD(4, true); break;
        }
    } else {
        if (c.ns == 1) FEDM_PHOTO_LOAD(1, false);
        else FEDM_PHOTO_LOAD(2, false);
    }
#undef FEDM_PHOTO_LOAD
    hipLaunchKernelGGL(photo_vertex_sum_kernel, gv, b, 0, c.stream, c.nv, c.nvp, ph.v_ptr, ph.v_idx, ph.zero, ph.cell_g,
                       ph.g);
}

// ---- source tables -----------------------------------------------------------------------------
struct PhotoTables {
    double *ext[FEDM_MAX_SPECIES];   // null: not a target
    double c[PHOTO_MAX_TERMS];
};

// A thread per cell: ext[cell][a] = sum_m c_m y_m[vertex a], terms in ascending order, products rounded before they are
// added (no contraction: the value is the one the same sum gives on the host)
__global__ __launch_bounds__(256) void photo_table_kernel(int nc, int nvp, int n_terms, const int *__restrict__ cells,
                                                          const double *__restrict__ y, PhotoTables t) {
#pragma clang fp contract(off)
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= nc) return;
    double s[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int v = cells[3 * cell + a];
        double acc = 0.0;
        for (int m = 0; m < n_terms; ++m) acc += t.c[m] * y[(size_t)m * nvp + v];
        s[a] = acc;
    }
#pragma unroll
    for (int sp = 0; sp < FEDM_MAX_SPECIES; ++sp) {
        if (!t.ext[sp]) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) t.ext[sp][3 * (size_t)cell + a] = s[a];
    }
}

void launch_photo_table_write(Ctx &c) {
    Photo &ph = *c.photo;
    PhotoTables t{};
    for (int s = 0; s < FEDM_MAX_SPECIES; ++s)
        t.ext[s] = (s < c.ns && ((ph.desc.target_species_mask >> s) & 1u)) ? c.d_ext[s] : nullptr;
    for (int m = 0; m < ph.desc.n_terms; ++m) t.c[m] = ph.desc.c[m];
    hipLaunchKernelGGL(photo_table_kernel, dim3((c.nc + 255) / 256), dim3(256), 0, c.stream, c.nc, c.nvp, ph.desc.n_terms,
                       c.d_cells, ph.y, t);
}

// ---- conjugate gradients on one scalar operator ----------------------------------------------------
// Sum over the workgroup in a fixed order (lanes by shuffles, then the four waves one after the other); the result
// is valid in thread 0.
__device__ __forceinline__ double photo_block_sum(double v, double *lds) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += lds[w];
    __syncthreads();
    return s;
}

// first pass of K <= 2 inner products: partials[k][workgroup]
template <int K>
__global__ __launch_bounds__(256) void photo_dots_kernel(int n, const double *__restrict__ a0, const double *__restrict__ b0,
                                                         const double *__restrict__ a1, const double *__restrict__ b1,
                                                         int slot0, double *__restrict__ partials) {
    __shared__ double lds[4];
    double s0 = 0.0, s1 = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        s0 += a0[i] * b0[i];
        if (K > 1) s1 += a1[i] * b1[i];
    }
    s0 = photo_block_sum(s0, lds);
    if (K > 1) s1 = photo_block_sum(s1, lds);
    if (threadIdx.x == 0) {
        partials[(size_t)slot0 * PHOTO_RED_BLOCKS + blockIdx.x] = s0;
        if (K > 1) partials[(size_t)(slot0 + 1) * PHOTO_RED_BLOCKS + blockIdx.x] = s1;
    }
}

// second pass, one workgroup: red[k] = sum over the workgroups of the first
__global__ __launch_bounds__(256) void photo_reduce_kernel(int nblocks, int k, const double *__restrict__ partials,
                                                           double *__restrict__ red) {
    __shared__ double lds[4];
    for (int j = 0; j < k; ++j) {
        const double v = (int)threadIdx.x < nblocks ? partials[(size_t)j * PHOTO_RED_BLOCKS + threadIdx.x] : 0.0;
        const double s = photo_block_sum(v, lds);
        if (threadIdx.x == 0) red[j] = s;
    }
}

// x += alpha p, r -= alpha q, partials[0] of r.r; JACOBI: z = dinv r and partials[1] of r.z as well
template <bool JACOBI>
__global__ __launch_bounds__(256) void photo_cg_update_kernel(int n, double alpha, const double *__restrict__ p,
                                                              const double *__restrict__ q, double *__restrict__ x,
                                                              double *__restrict__ r, const double *__restrict__ dinv,
                                                              double *__restrict__ z, double *__restrict__ partials) {
    __shared__ double lds[4];
    double s0 = 0.0, s1 = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * q[i];
        r[i] = ri;
        s0 += ri * ri;
        if (JACOBI) {
            const double zi = dinv[i] * ri;
            z[i] = zi;
            s1 += ri * zi;
        }
    }
    s0 = photo_block_sum(s0, lds);
    if (JACOBI) s1 = photo_block_sum(s1, lds);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s0;
        if (JACOBI) partials[PHOTO_RED_BLOCKS + blockIdx.x] = s1;
    }
}

__global__ void photo_jacobi_kernel(int n, const double *__restrict__ dinv, const double *__restrict__ r,
                                    double *__restrict__ z) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) z[i] = dinv[i] * r[i];
}

// p = z + beta p
__global__ void photo_direction_kernel(int n, const double *__restrict__ z, double beta, double *__restrict__ p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = z[i] + beta * p[i];
}

ScalarCgResult scalar_pcg(Ctx &c, const EllMat &A, Amg *M, const double *b, double *x, double rtol, int max_it) {
    Photo &ph = *c.photo;
    const int n = A.n_rows_p;
    const int red_grid = std::min((n + 255) / 256, PHOTO_RED_BLOCKS);
    const dim3 gv((n + 255) / 256), gr(red_grid), bl(256);
    // with a hierarchy the residual lives in its finest right-hand side and z is the cycle's result: no copies
    double *r = M ? M->levels[0].b : ph.r, *z = M ? M->levels[0].x : ph.z, *p = ph.p, *q = ph.q;
    auto read = [&](int k) {
        hipLaunchKernelGGL(photo_reduce_kernel, dim3(1), bl, 0, c.stream, red_grid, k, ph.partials, ph.red);
        wait_red_seq(c, publish_values(c, ph.red, k));
    };
    auto precondition = [&] {   // z = Minv r
        if (M) {
            M->vcycle(c, 0, 0);
            ++ph.stats[PH_VCYCLES];
        } else {
            hipLaunchKernelGGL(photo_jacobi_kernel, gv, bl, 0, c.stream, n, A.dinv, r, z);
        }
    };
    ell_apply(c, A, 1, x, b, r, 0.0);   // r = b - A x
    hipLaunchKernelGGL(photo_dots_kernel<2>, gr, bl, 0, c.stream, n, b, b, r, r, 0, ph.partials);
    read(2);
    const double bnorm = std::sqrt(c.h_red[0]);
    double rn = std::sqrt(c.h_red[1]);
    if (!std::isfinite(bnorm) || !std::isfinite(rn)) return ScalarCgResult{0, bnorm, rn};
    if (bnorm == 0.0) {   // the solution is 0, whatever the start
        hipMemsetAsync(x, 0, sizeof(double) * n, c.stream);
        return ScalarCgResult{0, 0.0, 0.0};
    }
    const double tol = rtol * bnorm;
    if (rn <= tol) return ScalarCgResult{0, bnorm, rn};
    precondition();
    hipLaunchKernelGGL(photo_dots_kernel<1>, gr, bl, 0, c.stream, n, r, z, r, z, 0, ph.partials);
    read(1);
    double rz = c.h_red[0];
    hipMemcpyAsync(p, z, sizeof(double) * n, hipMemcpyDeviceToDevice, c.stream);
    int it = 0;
    while (it < max_it) {
        ell_apply(c, A, 0, p, nullptr, q, 0.0);
        hipLaunchKernelGGL(photo_dots_kernel<1>, gr, bl, 0, c.stream, n, p, q, p, q, 0, ph.partials);
        read(1);
        const double pq = c.h_red[0];
        const double alpha = rz / pq;
        if (!std::isfinite(alpha) || pq <= 0.0) {   // not positive definite, or a NaN on the way
            rn = std::nan("");
            break;
        }
        if (M) {
            hipLaunchKernelGGL(photo_cg_update_kernel<false>, gr, bl, 0, c.stream, n, alpha, p, q, x, r, A.dinv, z,
                               ph.partials);
            precondition();
            hipLaunchKernelGGL(photo_dots_kernel<1>, gr, bl, 0, c.stream, n, r, z, r, z, 1, ph.partials);
        } else {
            hipLaunchKernelGGL(photo_cg_update_kernel<true>, gr, bl, 0, c.stream, n, alpha, p, q, x, r, A.dinv, z,
                               ph.partials);
        }
        read(2);
        rn = std::sqrt(c.h_red[0]);
        const double rz_new = c.h_red[1];
        ++it;
        if (!std::isfinite(rn) || rn <= tol) break;
        hipLaunchKernelGGL(photo_direction_kernel, gv, bl, 0, c.stream, n, z, rz_new / rz, p);
        rz = rz_new;
    }
    return ScalarCgResult{it, bnorm, rn};
}

}  // namespace fedm
