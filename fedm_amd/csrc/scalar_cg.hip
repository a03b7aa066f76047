// Conjugate gradients on one scalar operator (scalar_cg.hpp).  Plain launches on the context's stream; no kernel waits
// for another workgroup and none adds with atomics: every sum has a fixed order, so a solve is bitwise reproducible.
#include "scalar_cg.hpp"

#include <algorithm>

#include "postproc.hpp"

namespace fedm {

void ScalarCgWork::release() {
    void *ptrs[] = {r, z, p, q, partials, red};
    for (void *v : ptrs)
        if (v) hipFree(v);
    r = z = p = q = partials = red = nullptr;
}

int ScalarCgWork::alloc(size_t nvp) {
    if (device_array<double>(r, nullptr, nvp) || device_array<double>(z, nullptr, nvp) ||
        device_array<double>(p, nullptr, nvp) || device_array<double>(q, nullptr, nvp) ||
        device_array<double>(partials, nullptr, (size_t)2 * SCALAR_CG_RED_BLOCKS) ||
        device_array<double>(red, nullptr, 4)) {
        release();
        return -1;
    }
    return 0;
}

// Sum over the workgroup in a fixed order (lanes by shuffles, then the four waves one after the other); the result
// is valid in thread 0.
__device__ __forceinline__ double scalar_cg_block_sum(double v, double *lds) {
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
__global__ __launch_bounds__(256) void scalar_cg_dots_kernel(int n, const double *__restrict__ a0,
                                                             const double *__restrict__ b0, const double *__restrict__ a1,
                                                             const double *__restrict__ b1, int slot0,
                                                             double *__restrict__ partials) {
    __shared__ double lds[4];
    double s0 = 0.0, s1 = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        s0 += a0[i] * b0[i];
        if (K > 1) s1 += a1[i] * b1[i];
    }
    s0 = scalar_cg_block_sum(s0, lds);
    if (K > 1) s1 = scalar_cg_block_sum(s1, lds);
    if (threadIdx.x == 0) {
        partials[(size_t)slot0 * SCALAR_CG_RED_BLOCKS + blockIdx.x] = s0;
        if (K > 1) partials[(size_t)(slot0 + 1) * SCALAR_CG_RED_BLOCKS + blockIdx.x] = s1;
    }
}

// second pass, one workgroup: red[k] = sum over the workgroups of the first
__global__ __launch_bounds__(256) void scalar_cg_reduce_kernel(int nblocks, int k, const double *__restrict__ partials,
                                                               double *__restrict__ red) {
    __shared__ double lds[4];
    for (int j = 0; j < k; ++j) {
        const double v = (int)threadIdx.x < nblocks ? partials[(size_t)j * SCALAR_CG_RED_BLOCKS + threadIdx.x] : 0.0;
        const double s = scalar_cg_block_sum(v, lds);
        if (threadIdx.x == 0) red[j] = s;
    }
}

// x += alpha p, r -= alpha q, partials[0] of r.r; JACOBI: z = dinv r and partials[1] of r.z as well
template <bool JACOBI>
__global__ __launch_bounds__(256) void scalar_cg_update_kernel(int n, double alpha, const double *__restrict__ p,
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
    s0 = scalar_cg_block_sum(s0, lds);
    if (JACOBI) s1 = scalar_cg_block_sum(s1, lds);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s0;
        if (JACOBI) partials[SCALAR_CG_RED_BLOCKS + blockIdx.x] = s1;
    }
}

__global__ void scalar_cg_jacobi_kernel(int n, const double *__restrict__ dinv, const double *__restrict__ r,
                                        double *__restrict__ z) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) z[i] = dinv[i] * r[i];
}

// p = z + beta p
__global__ void scalar_cg_direction_kernel(int n, const double *__restrict__ z, double beta, double *__restrict__ p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = z[i] + beta * p[i];
}

ScalarCgResult scalar_pcg(Ctx &c, ScalarCgWork &w, const EllMat &A, Amg *M, const double *b, double *x, double rtol,
                          int max_it) {
    const int n = A.n_rows_p;
    const int red_grid = std::min((n + 255) / 256, SCALAR_CG_RED_BLOCKS);
    const dim3 gv((n + 255) / 256), gr(red_grid), bl(256);
    // with a hierarchy the residual lives in its finest right-hand side and z is the cycle's result: no copies
    double *r = M ? M->levels[0].b : w.r, *z = M ? M->levels[0].x : w.z, *p = w.p, *q = w.q;
    int vcycles = 0;
    auto read = [&](int k) {
        hipLaunchKernelGGL(scalar_cg_reduce_kernel, dim3(1), bl, 0, c.stream, red_grid, k, w.partials, w.red);
        wait_red_seq(c, publish_values(c, w.red, k));
    };
    auto precondition = [&] {   // z = Minv r
        if (M) {
            M->vcycle(c, 0, 0);
            ++vcycles;
        } else {
            hipLaunchKernelGGL(scalar_cg_jacobi_kernel, gv, bl, 0, c.stream, n, A.dinv, r, z);
        }
    };
    ell_apply(c, A, 1, x, b, r, 0.0);   // r = b - A x
    hipLaunchKernelGGL(scalar_cg_dots_kernel<2>, gr, bl, 0, c.stream, n, b, b, r, r, 0, w.partials);
    read(2);
    const double bnorm = std::sqrt(c.h_red[0]);
    double rn = std::sqrt(c.h_red[1]);
    if (!std::isfinite(bnorm) || !std::isfinite(rn)) return ScalarCgResult{0, bnorm, rn, 0};
    if (bnorm == 0.0) {   // the solution is 0, whatever the start
        hipMemsetAsync(x, 0, sizeof(double) * n, c.stream);
        return ScalarCgResult{0, 0.0, 0.0, 0};
    }
    const double tol = rtol * bnorm;
    if (rn <= tol) return ScalarCgResult{0, bnorm, rn, 0};
    precondition();
    hipLaunchKernelGGL(scalar_cg_dots_kernel<1>, gr, bl, 0, c.stream, n, r, z, r, z, 0, w.partials);
    read(1);
    double rz = c.h_red[0];
    hipMemcpyAsync(p, z, sizeof(double) * n, hipMemcpyDeviceToDevice, c.stream);
    int it = 0;
    while (it < max_it) {
        ell_apply(c, A, 0, p, nullptr, q, 0.0);
        hipLaunchKernelGGL(scalar_cg_dots_kernel<1>, gr, bl, 0, c.stream, n, p, q, p, q, 0, w.partials);
        read(1);
        const double pq = c.h_red[0];
        const double alpha = rz / pq;
        if (!std::isfinite(alpha) || pq <= 0.0) {   // not positive definite, or a NaN on the way
            rn = std::nan("");
            break;
        }
        if (M) {
            hipLaunchKernelGGL(scalar_cg_update_kernel<false>, gr, bl, 0, c.stream, n, alpha, p, q, x, r, A.dinv, z,
                               w.partials);
            precondition();
            hipLaunchKernelGGL(scalar_cg_dots_kernel<1>, gr, bl, 0, c.stream, n, r, z, r, z, 1, w.partials);
        } else {
            hipLaunchKernelGGL(scalar_cg_update_kernel<true>, gr, bl, 0, c.stream, n, alpha, p, q, x, r, A.dinv, z,
                               w.partials);
        }
        read(2);
        rn = std::sqrt(c.h_red[0]);
        const double rz_new = c.h_red[1];
        ++it;
        if (!std::isfinite(rn) || rn <= tol) break;
        hipLaunchKernelGGL(scalar_cg_direction_kernel, gv, bl, 0, c.stream, n, z, rz_new / rz, p);
        rz = rz_new;
    }
    return ScalarCgResult{it, bnorm, rn, vcycles};
}

}  // namespace fedm
