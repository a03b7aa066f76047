// Reductions, the host mailbox and the vector kernels of the FEDM hot path (gfx950, fp64, HBM-bound): dots_* and the
// reduce_* / *_finish kernels, publish, Gram-Schmidt updates (cgs_*, the field-split first stage fused in), wait_red /
// norm2_* / read_red / publish_values, axpy and friends, the Newton update, the field error and the copy-bandwidth
// probe.  The element assembly lives in assemble.hip and assemble3.hip, the matrix side (block inverse, SpMV, SpMV
// fused with dots) in spmv.hip.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>

#include "comm.hpp"
#include "device_util.hpp"
#include "fedm_internal.hpp"

namespace fedm {

// =============================================================================================
// Reductions: deterministic two-stage (per-block partials in a fixed grid, then one block).
// =============================================================================================
template <int K>
__device__ __forceinline__ void block_reduce_store(double (&acc)[K], double *partials, int kbase) {
    __shared__ double sm[4][K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double s = wave_sum(acc[i]);
        if (lane == 0) sm[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const double s = sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] + sm[3][threadIdx.x];
        partials[PARTIAL_AT(blockIdx.x, kbase + threadIdx.x)] = s;
    }
}

// partials[block][kbase + i] = sum over the block's grid-stride range of xs[i] * y
// W (row-equilibrated GMRES, fedm_set_krylov_scaling): the sums run in the inner product <x, y> = sum_i wgt_i x_i y_i,
// wgt = d^2 of row_scale_kernel.  A template flag: the unweighted instantiation is the code it was.
template <int K, bool W>
__device__ __forceinline__ void dots_block(const PtrPack8 &xs, const double *__restrict__ y, size_t n,
                                           double *__restrict__ partials, int kbase, const double *__restrict__ wgt) {
    double acc[K];
#pragma unroll
    for (int i = 0; i < K; ++i) acc[i] = 0.0;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
         idx += (size_t)gridDim.x * blockDim.x) {
        const double yv = W ? y[idx] * wgt[idx] : y[idx];
#pragma unroll
        for (int i = 0; i < K; ++i) acc[i] += xs.p[i][idx] * yv;
    }
    block_reduce_store<K>(acc, partials, kbase);
}

template <int K, bool W = false>
__global__ __launch_bounds__(256) void dots_kernel(PtrPack8 xs, const double *__restrict__ y,
                                                   size_t n, double *__restrict__ partials, int kbase,
                                                   const double *__restrict__ wgt = nullptr) {
    dots_block<K, W>(xs, y, n, partials, kbase, wgt);
}

// ---- the second Gram-Schmidt pass of a refined Krylov step (krylov.cpp), queued behind the step's first pass --------
// Three kernels that read red[RED_REFINE], written by the step's first finish (spmv_dots_finish_kernel, finish = 2):
// 0, the first pass was sound -- the reduction and the update return at once and touch nothing, the finish publishes
// what the first finish left; 1, strong cancellation -- t = w - V h was left unscaled:
//   dots_refine_kernel    c_i = v_i . t (i < k - 1) and tt = t . t, per-block partials like dots_kernel;
//   refine_finish_kernel  hn2' = tt - sum c_i^2 (the c_i are rounding-sized beside |t|: no cancellation), scale' =
//                         1 / sqrt(hn2'); red[i] = h_i + c_i, red[k-1] = hn2', red[RED_REFINE] = 1 (refined) or 2 (hn2'
//                         fails the test against tt in its turn: scale' = 1, the host refines as it always did);
//                         coef[i] = c_i and coef[RED_K-1] = scale' for the update; the step's ONE publication;
//   cgs_refine_fs_kernel  cgs_update_fs_kernel on t with those coefficients.
template <int K, bool W = false>
__global__ __launch_bounds__(256) void dots_refine_kernel(PtrPack8 xs, const double *__restrict__ y, size_t n,
                                                          double *__restrict__ partials,
                                                          const double *__restrict__ red,
                                                          const double *__restrict__ wgt = nullptr) {
    if (red[RED_REFINE] == 0.0) return;
    dots_block<K, W>(xs, y, n, partials, 0, wgt);
}

__global__ __launch_bounds__(1024) void refine_finish_kernel(const double *__restrict__ partials, int nblocks, int k,
                                                            double *__restrict__ red, double *__restrict__ coef,
                                                            double *mail, unsigned long long *seq) {
    __shared__ double fin[RED_K];
    __shared__ double cs[RED_K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < RED_K) fin[threadIdx.x] = red[threadIdx.x];
    __syncthreads();
    if (fin[RED_REFINE] != 0.0) {   // (the same for every thread)
        for (int i = wave; i < k; i += 16) {
            double sum = 0.0;
            for (int b = lane; b < nblocks; b += 64) sum += partials[PARTIAL_AT(b, i)];
            sum = wave_sum(sum);
            if (lane == 0) cs[i] = sum;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double tt = cs[k - 1];
            double cc = 0.0;
            for (int i = 0; i < k - 1; ++i) cc += cs[i] * cs[i];
            const double hn2 = tt - cc;
            const bool sound = hn2 > 1e-8 * tt && hn2 > 0.0;
            const double scale = sound ? 1.0 / sqrt(hn2) : 1.0;
            for (int i = 0; i < k - 1; ++i) {
                fin[i] += cs[i];
                coef[i] = cs[i];
            }
            fin[k - 1] = hn2;
            fin[RED_K - 1] = scale;
            coef[RED_K - 1] = scale;
            fin[RED_REFINE] = sound ? 1.0 : 2.0;
        }
        __syncthreads();
    }
    if (threadIdx.x < 64) {
        const unsigned long long tag = *seq + 1;
        double *slot = mail + (tag & (MAIL_SLOTS - 1)) * (RED_K + 1);
        for (int i = threadIdx.x; i < RED_K; i += 64) {
            red[i] = fin[i];
            slot[i] = fin[i];
        }
        __threadfence_system();
        if (threadIdx.x == 0) {
            *seq = tag;
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(slot + RED_K), tag, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

__global__ void reduce_partials_kernel(const double *__restrict__ partials, int nblocks, int k,
                                       double *__restrict__ out) {
    // one wave per output; fixed summation order
    const int i = blockIdx.x;
    if (i >= k) return;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) s += partials[PARTIAL_AT(b, i)];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[i] = s;
}

// GMRES orthogonalisation step in ONE reduction: the dots kernel has produced h_i = v_i . w
// (i < k-1) and ww = w . w (slot k-1); after the (all-)reduction one thread derives
// |w - sum h_i v_i|^2 = ww - sum h_i^2 (Pythagoras; V orthonormal).
// out[k-1] <- that squared norm, out[RED_K-2] <- ww, out[RED_K-1] <- scale for the update
// (1/norm, or 1 when cancellation is too strong to trust the formula -> host refines).
// Results go to the host through a mailbox in host-mapped pinned memory: values, a system-scope
// fence, then the sequence tag the host polls (wait_red) -- no copy kernel, no stream
// synchronisation, and the host can queue the next iteration while this one finishes.
// The tag is a launch counter kept in device memory (a replayed graph has fixed arguments).
__device__ __forceinline__ void publish(const double *__restrict__ red, int k, double *mail,
                                        unsigned long long *seq) {
    // one wave; MAIL_SLOTS mailbox slots, chosen by the tag's low bits: the host may still be reading
    // publication n when n+1 and n+2 (Krylov steps launched ahead) arrive
    const unsigned long long tag = *seq + 1;
    double *slot = mail + (tag & (MAIL_SLOTS - 1)) * (RED_K + 1);
    for (int i = threadIdx.x; i < k; i += 64) slot[i] = red[i];
    __threadfence_system();
    if (threadIdx.x == 0) {
        *seq = tag;
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(slot + RED_K), tag, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(64) void publish_kernel(const double *__restrict__ red, int k, double *mail,
                                                     unsigned long long *seq) {
    publish(red, k, mail, seq);
}

__global__ __launch_bounds__(64) void cgs_finish_kernel(int k, double *__restrict__ out, double *mail,
                                                        unsigned long long *seq) {
    if (threadIdx.x == 0) {
        const double ww = out[k - 1];
        double hh = 0.0;
        for (int i = 0; i < k - 1; ++i) hh += out[i] * out[i];
        const double hn2 = ww - hh;
        out[RED_K - 2] = ww;
        out[k - 1] = hn2;
        out[RED_K - 1] = (hn2 > 1e-8 * ww && hn2 > 0.0) ? 1.0 / sqrt(hn2) : 1.0;
    }
    __syncthreads();
    publish(out, RED_K, mail, seq);
}

// Single-GPU Krylov step, two kernels instead of five:
//  dots_scatter_kernel  finishes the preconditioner (the potential component of y is taken from
//                       the V-cycle result x0 and stored into y: replaces fs_scatter_kernel) and
//                       forms the per-block partial dot products like dots_kernel;
//  reduce_finish_kernel reduces the partials of all k slots in the fixed order of
//                       reduce_partials_kernel, applies the cgs_finish_kernel formulae and
//                       publishes to the host mailbox.
// Every kernel boundary costs ~4-5 us on this GPU, more than the work of these small kernels.
// (A single kernel with a last-block-done ticket was tried: the agent-scope fences it needs
// across the 8 XCDs' L2s cost 60 us.)
template <int K, bool W = false>
__global__ __launch_bounds__(256) void dots_scatter_kernel(PtrPack8 xs, double *__restrict__ y, size_t n,
                                                           double *__restrict__ partials, int kbase,
                                                           int self_index, const double *__restrict__ x0,
                                                           int neq, const double *__restrict__ wgt = nullptr) {
    double acc[K];
#pragma unroll
    for (int i = 0; i < K; ++i) acc[i] = 0.0;
    if (x0) {
        // one vertex per thread: its potential component comes from x0 and is stored into y
        const size_t nvert = n / (size_t)neq;
        for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvert;
             v += (size_t)gridDim.x * blockDim.x) {
            const size_t base = v * neq;
            const double phi = x0[v];
            y[base + neq - 1] = phi;
            for (int cidx = 0; cidx < neq; ++cidx) {
                const double yv = (cidx == neq - 1) ? phi : y[base + cidx];
                const double yw = W ? yv * wgt[base + cidx] : yv;
#pragma unroll
                for (int i = 0; i < K; ++i) acc[i] += (i == self_index ? yv : xs.p[i][base + cidx]) * yw;
            }
        }
    } else {
        for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
             idx += (size_t)gridDim.x * blockDim.x) {
            const double yv = y[idx];
            const double yw = W ? yv * wgt[idx] : yv;
#pragma unroll
            for (int i = 0; i < K; ++i) acc[i] += (i == self_index ? yv : xs.p[i][idx]) * yw;
        }
    }
    block_reduce_store<K>(acc, partials, kbase);
}

__global__ __launch_bounds__(1024) void reduce_finish_kernel(const double *__restrict__ partials, int nblocks,
                                                            int k, double *__restrict__ out, double *mail,
                                                            unsigned long long *seq) {
    __shared__ double fin[RED_K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < RED_K) fin[threadIdx.x] = (threadIdx.x == RED_SPARE) ? out[RED_SPARE] : 0.0;
    __syncthreads();
    // 16 waves, one slot each per pass: a Krylov step's j + 2 slots finish in one or two passes
    for (int i = wave; i < k; i += 16) {
        double sum = 0.0;
        for (int b = lane; b < nblocks; b += 64) sum += partials[PARTIAL_AT(b, i)];
        sum = wave_sum(sum);
        if (lane == 0) fin[i] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double ww = fin[k - 1];
        double hh = 0.0;
        for (int i = 0; i < k - 1; ++i) hh += fin[i] * fin[i];
        const double hn2 = ww - hh;
        fin[RED_K - 2] = ww;
        fin[k - 1] = hn2;
        fin[RED_K - 1] = (hn2 > 1e-8 * ww && hn2 > 0.0) ? 1.0 / sqrt(hn2) : 1.0;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const unsigned long long tag = *seq + 1;
        double *slot = mail + (tag & (MAIL_SLOTS - 1)) * (RED_K + 1);
        for (int i = threadIdx.x; i < RED_K; i += 64) {
            out[i] = fin[i];
            slot[i] = fin[i];
        }
        __threadfence_system();
        if (threadIdx.x == 0) {
            *seq = tag;
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(slot + RED_K), tag, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <int K, bool FINAL>
__global__ void cgs_update_kernel(size_t n, const double *__restrict__ coef, int base, PtrPack8 xs,
                                  double *__restrict__ y) {
    double cf[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cf[k] = coef[base + k];
    const double scale = FINAL ? coef[RED_K - 1] : 1.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double s = y[i];
#pragma unroll
        for (int k = 0; k < K; ++k) s -= cf[k] * xs.p[k][i];
        y[i] = FINAL ? s * scale : s;
    }
}

static dim3 vec_grid(const Ctx &c);

static int red_grid(const Ctx &c) {
    const size_t blocks = ((size_t)c.n_dot + 255) / 256;
    return (int)(blocks < (size_t)RED_BLOCKS ? blocks : (size_t)RED_BLOCKS);
}

void launch_dots(Ctx &c, const double *const *xs, const double *y, int k, bool finish) {
    const int grid = red_grid(c);
    int done = 0;
    while (done < k) {
        const int kk = (k - done) >= 8 ? 8 : (k - done);
        PtrPack8 pk;
        for (int i = 0; i < 8; ++i) pk.p[i] = xs[done + (i < kk ? i : 0)];
#define FEDM_D(K)                                                                                              \
    if (c.red_w) hipLaunchKernelGGL((dots_kernel<K, true>), dim3(grid), dim3(256), 0, c.stream, pk, y,             \
                                    (size_t)c.n_dot, c.d_partials, done, c.red_w);                                 \
    else hipLaunchKernelGGL(dots_kernel<K>, dim3(grid), dim3(256), 0, c.stream, pk, y, (size_t)c.n_dot, c.d_partials, done)
        switch (kk) {
            case 1: FEDM_D(1); break;
            case 2: FEDM_D(2); break;
            case 3: FEDM_D(3); break;
            case 4: FEDM_D(4); break;
            case 5: FEDM_D(5); break;
            case 6: FEDM_D(6); break;
            case 7: FEDM_D(7); break;
            default: FEDM_D(8); break;
        }
#undef FEDM_D
        done += kk;
    }
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(k), dim3(64), 0, c.stream, c.d_partials, grid, k, c.d_red);
    comm_allreduce(c, c.d_red, k);
    if (finish) {
        hipLaunchKernelGGL(cgs_finish_kernel, dim3(1), dim3(64), 0, c.stream, k, c.d_red, c.h_mail,
                           c.d_mail_seq);
        if (!c.capturing) ++c.mail_seq;  // a captured launch counts when its graph is launched
    }
}

// single-GPU Krylov step: dots (+ the scatter of the V-cycle result x0 into the potential
// component of y), then reduction + finish + publication
void launch_cgs_finish(Ctx &c, int k) {
    hipLaunchKernelGGL(cgs_finish_kernel, dim3(1), dim3(64), 0, c.stream, k, c.d_red, c.h_mail, c.d_mail_seq);
    if (!c.capturing) ++c.mail_seq;
}

// finish = false (several GPUs): only the local sums, d_red[0..k), for the all-reduce that follows
void launch_dots_fused(Ctx &c, const double *const *xs, double *y, int k, const double *x0, bool finish) {
    const int grid = red_grid(c);
    int done = 0;
    while (done < k) {
        const int kk = (k - done) >= 8 ? 8 : (k - done);
        PtrPack8 pk;
        int self = -1;
        for (int i = 0; i < 8; ++i) {
            pk.p[i] = xs[done + (i < kk ? i : 0)];
            if (i < kk && pk.p[i] == y) self = i;
        }
        const double *sc = (done == 0) ? x0 : nullptr;
#define FEDM_DF(K)                                                                                     \
    if (c.red_w) hipLaunchKernelGGL((dots_scatter_kernel<K, true>), dim3(grid), dim3(256), 0, c.stream, pk, y, \
                                    (size_t)c.n_dot, c.d_partials, done, self, sc, c.neq, c.red_w);        \
    else hipLaunchKernelGGL(dots_scatter_kernel<K>, dim3(grid), dim3(256), 0, c.stream, pk, y, (size_t)c.n_dot, \
                            c.d_partials, done, self, sc, c.neq)
        switch (kk) {
            case 1: FEDM_DF(1); break;
            case 2: FEDM_DF(2); break;
            case 3: FEDM_DF(3); break;
            case 4: FEDM_DF(4); break;
            case 5: FEDM_DF(5); break;
            case 6: FEDM_DF(6); break;
            case 7: FEDM_DF(7); break;
            default: FEDM_DF(8); break;
        }
#undef FEDM_DF
        done += kk;
    }
    if (!finish) {
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(k), dim3(64), 0, c.stream, c.d_partials, grid, k, c.d_red);
        return;
    }
    hipLaunchKernelGGL(reduce_finish_kernel, dim3(1), dim3(1024), 0, c.stream, c.d_partials, grid, k, c.d_red,
                       c.h_mail, c.d_mail_seq);
    if (!c.capturing) ++c.mail_seq;
}

// y = (y - sum_i d_red[i] xs[i]) * d_red[RED_K-1], coefficients stay on the device
void launch_cgs_update(Ctx &c, int k, const double *const *xs, double *y) {
    int done = 0;
    while (done < k) {
        const int kk = (k - done) >= 8 ? 8 : (k - done);
        const bool fin = (done + kk == k);
        PtrPack8 pk;
        for (int i = 0; i < 8; ++i) pk.p[i] = xs[done + (i < kk ? i : 0)];
#define FEDM_CGS(K)                                                                               \
    if (fin) hipLaunchKernelGGL((cgs_update_kernel<K, true>), vec_grid(c), dim3(256), 0, c.stream, \
                                (size_t)c.np, c.d_red, done, pk, y);                               \
    else hipLaunchKernelGGL((cgs_update_kernel<K, false>), vec_grid(c), dim3(256), 0, c.stream,     \
                            (size_t)c.np, c.d_red, done, pk, y);
        switch (kk) {
            case 1: FEDM_CGS(1) break;
            case 2: FEDM_CGS(2) break;
            case 3: FEDM_CGS(3) break;
            case 4: FEDM_CGS(4) break;
            case 5: FEDM_CGS(5) break;
            case 6: FEDM_CGS(6) break;
            case 7: FEDM_CGS(7) break;
            default: FEDM_CGS(8) break;
        }
#undef FEDM_CGS
        done += kk;
    }
}

// One GPU, field split on the right with species sweeps: whoever completes a Krylov vector v_j also forms the first
// stage of the preconditioner's application to it -- g = Duu^-1 v_u (single precision, what the sweeps start from)
// and b0 = v_phi (the multigrid's right-hand side) -- while the vector's entries are in registers: the pointwise
// fs_species_kernel (amg.hip; 5.5 us of launch latency per Krylov step) is gone.  Same operations in the same
// order as cgs_update_kernel / scale_copy_kernel followed by fs_species_kernel.
template <int NS>
__device__ __forceinline__ void first_stage_of(int v, const double (&tv)[NS + 1], const double *__restrict__ dinv_uu,
                                               float *__restrict__ g32, double *__restrict__ b0) {
    const double *dp = dinv_uu + (size_t)(v >> 6) * NS * NS * SLICE + (v & 63);
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int cidx = 0; cidx < NS; ++cidx) acc += dp[(size_t)(r * NS + cidx) * SLICE] * tv[cidx];
        g32[(size_t)v * NS + r] = (float)acc;
    }
    b0[v] = tv[NS];
}

template <int K, int NS>
__device__ __forceinline__ void cgs_update_fs_block(int nvp, const double *__restrict__ coef, const PtrPack8 &xs,
                                                    double *__restrict__ y, const double *__restrict__ dinv_uu,
                                                    float *__restrict__ g32, double *__restrict__ b0) {
    constexpr int NEQ = NS + 1;
    double cf[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cf[k] = coef[k];
    const double scale = coef[RED_K - 1];
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvp; v += gridDim.x * blockDim.x) {
        double tv[NEQ];
#pragma unroll
        for (int r = 0; r < NEQ; ++r) {
            const size_t i = (size_t)v * NEQ + r;
            double t = y[i];
#pragma unroll
            for (int k = 0; k < K; ++k) t -= cf[k] * xs.p[k][i];
            t *= scale;
            y[i] = t;
            tv[r] = t;
        }
        first_stage_of<NS>(v, tv, dinv_uu, g32, b0);
    }
}

template <int K, int NS>
__global__ __launch_bounds__(256) void cgs_update_fs_kernel(int nvp, const double *__restrict__ coef, PtrPack8 xs,
                                                            double *__restrict__ y,
                                                            const double *__restrict__ dinv_uu,
                                                            float *__restrict__ g32, double *__restrict__ b0) {
    cgs_update_fs_block<K, NS>(nvp, coef, xs, y, dinv_uu, g32, b0);
}

// the update of a refined step's second pass (dots_refine_kernel): nothing when the first pass was sound
template <int K, int NS>
__global__ __launch_bounds__(256) void cgs_refine_fs_kernel(int nvp, const double *__restrict__ red,
                                                            const double *__restrict__ coef, PtrPack8 xs,
                                                            double *__restrict__ y,
                                                            const double *__restrict__ dinv_uu,
                                                            float *__restrict__ g32, double *__restrict__ b0) {
    if (red[RED_REFINE] == 0.0) return;
    cgs_update_fs_block<K, NS>(nvp, coef, xs, y, dinv_uu, g32, b0);
}

template <int NS>
__global__ __launch_bounds__(256) void scale_copy_fs_kernel(int nvp, double a, const double *__restrict__ x,
                                                            double *__restrict__ y,
                                                            const double *__restrict__ dinv_uu,
                                                            float *__restrict__ g32, double *__restrict__ b0) {
    constexpr int NEQ = NS + 1;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvp; v += gridDim.x * blockDim.x) {
        double tv[NEQ];
#pragma unroll
        for (int r = 0; r < NEQ; ++r) {
            const size_t i = (size_t)v * NEQ + r;
            tv[r] = a * x[i];
            y[i] = tv[r];
        }
        first_stage_of<NS>(v, tv, dinv_uu, g32, b0);
    }
}

// false: no fused kernel for this case (the caller launches the two kernels)
bool launch_cgs_update_fs(Ctx &c, int k, const double *const *xs, double *y, float *g32, double *b0) {
    if (c.ns != 2 || k < 1 || k > 4) return false;
    PtrPack8 pk;
    for (int i = 0; i < 8; ++i) pk.p[i] = xs[i < k ? i : 0];
    const dim3 g((c.nvp + 255) / 256), b(256);
#define FEDM_CGSF(K)                                                                                             \
    hipLaunchKernelGGL((cgs_update_fs_kernel<K, 2>), g, b, 0, c.stream, c.nvp, c.d_red, pk, y, c.d_dinv, g32, b0)
    switch (k) {
        case 1: FEDM_CGSF(1); break;
        case 2: FEDM_CGSF(2); break;
        case 3: FEDM_CGSF(3); break;
        default: FEDM_CGSF(4); break;
    }
#undef FEDM_CGSF
    return true;
}

// The second pass behind step j's first pass and update (vs = {v_0 ... v_j}, t the step's vector, as its update left
// it): three launches and the step's publication.  false: not instantiated for this case, nothing launched.
bool cgs_refine_applicable(const Ctx &c, int j) { return c.ns == 2 && j >= 0 && j + 1 <= 4; }

bool launch_cgs_refine(Ctx &c, int j, const double *const *vs, double *t, float *g32, double *b0) {
    if (!cgs_refine_applicable(c, j)) return false;
    const int k = j + 2, grid = red_grid(c);
    PtrPack8 pk;
    for (int i = 0; i < 8; ++i) pk.p[i] = i < k - 1 ? vs[i] : t;
    double *coef = c.d_red + RED_K;
#define FEDM_DR(K)                                                                                                  \
    if (c.red_w) hipLaunchKernelGGL((dots_refine_kernel<K, true>), dim3(grid), dim3(256), 0, c.stream, pk, t,          \
                                    (size_t)c.n_dot, c.d_partials, c.d_red, c.red_w);                                \
    else hipLaunchKernelGGL(dots_refine_kernel<K>, dim3(grid), dim3(256), 0, c.stream, pk, t, (size_t)c.n_dot,       \
                            c.d_partials, c.d_red)
    switch (k) {
        case 2: FEDM_DR(2); break;
        case 3: FEDM_DR(3); break;
        case 4: FEDM_DR(4); break;
        default: FEDM_DR(5); break;
    }
#undef FEDM_DR
    hipLaunchKernelGGL(refine_finish_kernel, dim3(1), dim3(1024), 0, c.stream, c.d_partials, grid, k, c.d_red, coef,
                       c.h_mail, c.d_mail_seq);
    if (!c.capturing) ++c.mail_seq;
    const dim3 g((c.nvp + 255) / 256), b(256);
#define FEDM_CR(K)                                                                                                  \
    hipLaunchKernelGGL((cgs_refine_fs_kernel<K, 2>), g, b, 0, c.stream, c.nvp, c.d_red, coef, pk, t, c.d_dinv, g32, b0)
    switch (j + 1) {
        case 1: FEDM_CR(1); break;
        case 2: FEDM_CR(2); break;
        case 3: FEDM_CR(3); break;
        default: FEDM_CR(4); break;
    }
#undef FEDM_CR
    return true;
}

bool launch_scale_copy_fs(Ctx &c, double a, const double *x, double *y, float *g32, double *b0) {
    if (c.ns != 2) return false;
    hipLaunchKernelGGL(scale_copy_fs_kernel<2>, dim3((c.nvp + 255) / 256), dim3(256), 0, c.stream, c.nvp, a, x, y,
                       c.d_dinv, g32, b0);
    return true;
}

__global__ void reduce_partials_slot_kernel(const double *__restrict__ partials, int nblocks,
                                            int k_src, double *__restrict__ out, int slot) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) s += partials[PARTIAL_AT(b, k_src)];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[slot] = s;
}

void launch_norm2(Ctx &c, const double *x, int slot) {
    const int grid = red_grid(c);
    PtrPack8 pk;
    for (int i = 0; i < 8; ++i) pk.p[i] = x;
    if (c.red_w)   // inside a row-equilibrated GMRES solve: |D x|^2
        hipLaunchKernelGGL((dots_kernel<1, true>), dim3(grid), dim3(256), 0, c.stream, pk, x, (size_t)c.n_dot, c.d_partials, RED_K - 1, c.red_w);
    else
        hipLaunchKernelGGL(dots_kernel<1>, dim3(grid), dim3(256), 0, c.stream, pk, x, (size_t)c.n_dot, c.d_partials, RED_K - 1);
    hipLaunchKernelGGL(reduce_partials_slot_kernel, dim3(1), dim3(64), 0, c.stream, c.d_partials, grid, RED_K - 1, c.d_red, slot);
    comm_allreduce(c, c.d_red + slot, 1);
}

// wait for publication `seq` and point c.h_red at its slot
void wait_red_seq(Ctx &c, unsigned long long seq) {
    double *slot = c.h_mail + (seq & (MAIL_SLOTS - 1)) * (RED_K + 1);
    c.h_red = slot;
    const unsigned long long *tag = reinterpret_cast<const unsigned long long *>(slot + RED_K);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(tag, __ATOMIC_ACQUIRE) == seq) return;
        __builtin_ia32_pause();
        if ((spins & 0xffff) == 0xffff) {
            // a faulted or lost queue never publishes: fall back to the runtime's own wait
            const bool failed = hipStreamQuery(c.stream) != hipErrorNotReady &&
                                __atomic_load_n(tag, __ATOMIC_ACQUIRE) != seq;
            const bool late = std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120);
            // a peer that died leaves an RCCL kernel spinning on this stream: ask the communicator
            if (comm_poll_async_error(c)) {
                for (int i = 0; i < RED_K; ++i) slot[i] = std::nan("");
                return;
            }
            if (failed || late) {
                hipStreamSynchronize(c.stream);
                if (__atomic_load_n(tag, __ATOMIC_ACQUIRE) != seq) {
                    // (diagnostics of a publication that never came: expected tag, the tags in the mailbox, the
                    // device's counter)
                    unsigned long long dev_seq = 0;
                    hipMemcpy(&dev_seq, c.d_mail_seq, sizeof(dev_seq), hipMemcpyDeviceToHost);
                    std::fprintf(stderr, "fedm: publication %llu did not arrive (%s); mailbox tags", seq,
                                 failed ? "the queue is empty" : "waited 120 s");
                    for (int k = 0; k < MAIL_SLOTS; ++k)
                        std::fprintf(stderr, " %llu", *reinterpret_cast<const unsigned long long *>(
                                                          c.h_mail + (size_t)k * (RED_K + 1) + RED_K));
                    std::fprintf(stderr, ", host count %llu, device count %llu\n", c.mail_seq, dev_seq);
                    for (int i = 0; i < RED_K; ++i) slot[i] = std::nan("");
                }
                return;
            }
        }
    }
}

void wait_red(Ctx &c) { wait_red_seq(c, c.mail_seq); }

// |x|^2 into d_red[slot] and publication of d_red[0..k) in one go: on one GPU the reduction of the
// partial sums and the mailbox write are one kernel
__global__ __launch_bounds__(64) void reduce_slot_publish_kernel(const double *__restrict__ partials, int nblocks,
                                                                 int k_src, double *__restrict__ out, int slot,
                                                                 int k, double *mail, unsigned long long *seq) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) s += partials[PARTIAL_AT(b, k_src)];
    s = wave_sum(s);
    s = __shfl(s, 0, 64);
    if (threadIdx.x == 0) out[slot] = s;
    const unsigned long long tag = *seq + 1;
    double *m = mail + (tag & (MAIL_SLOTS - 1)) * (RED_K + 1);
    for (int i = threadIdx.x; i < k; i += 64) m[i] = (i == slot) ? s : out[i];
    __threadfence_system();
    if (threadIdx.x == 0) {
        *seq = tag;
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(m + RED_K), tag, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// |x|^2 into slot `slot` and d_red[0..k) into the mailbox, without the wait: the caller may queue
// more work behind the publication before it calls wait_red (what it queues runs while the
// numbers travel to the host)
void norm2_publish(Ctx &c, const double *x, int slot, int k, int k_sum) {
    if (c.comm) {  // the all-reduce sits between the reduction and the publication
        // k_sum > 1 (slot 0): d_red[1 .. k_sum) hold rank-local sums that have not been all-reduced yet
        // (|dx|^2, |x|^2 of the Newton update, the watched component's error sums): ONE all-reduce
        // carries them together with |x|^2 instead of one each
        if (slot == 0 && k_sum > 1) {
            const int grid = red_grid(c);
            PtrPack8 pk;
            for (int i = 0; i < 8; ++i) pk.p[i] = x;
            hipLaunchKernelGGL(dots_kernel<1>, dim3(grid), dim3(256), 0, c.stream, pk, x, (size_t)c.n_dot, c.d_partials, RED_K - 1);
            hipLaunchKernelGGL(reduce_partials_slot_kernel, dim3(1), dim3(64), 0, c.stream, c.d_partials, grid, RED_K - 1, c.d_red, 0);
            comm_allreduce(c, c.d_red, k_sum);
        } else {
            launch_norm2(c, x, slot);
        }
        hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, c.stream, c.d_red, k, c.h_mail, c.d_mail_seq);
        ++c.mail_seq;
        return;
    }
    const int grid = red_grid(c);
    PtrPack8 pk;
    for (int i = 0; i < 8; ++i) pk.p[i] = x;
    hipLaunchKernelGGL(dots_kernel<1>, dim3(grid), dim3(256), 0, c.stream, pk, x, (size_t)c.n_dot, c.d_partials, RED_K - 1);
    hipLaunchKernelGGL(reduce_slot_publish_kernel, dim3(1), dim3(64), 0, c.stream, c.d_partials, grid, RED_K - 1,
                       c.d_red, slot, k, c.h_mail, c.d_mail_seq);
    ++c.mail_seq;
}

void norm2_read(Ctx &c, const double *x, int slot, int k) {
    norm2_publish(c, x, slot, k, 1);
    wait_red(c);
}

// src[0 .. k) into the mailbox without the wait; the publication's sequence number (wait_red_seq)
unsigned long long publish_values(Ctx &c, const double *src, int k) {
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, c.stream, src, k, c.h_mail, c.d_mail_seq);
    return ++c.mail_seq;
}
// ... the launch alone (inside a stream capture: whoever replays the graph advances Ctx::mail_seq per replay)
void publish_values_queued(Ctx &c, const double *src, int k) {
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, c.stream, src, k, c.h_mail, c.d_mail_seq);
}

void read_red(Ctx &c, int k) {
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, c.stream, c.d_red, k, c.h_mail, c.d_mail_seq);
    ++c.mail_seq;
    wait_red(c);
}

// =============================================================================================
// Vector updates
// =============================================================================================
__global__ void axpy_kernel(size_t n, double a, const double *__restrict__ x, double *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] += a * x[i];
}
__global__ void scale_copy_kernel(size_t n, double a, const double *__restrict__ x, double *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = a * x[i];
}

static dim3 vec_grid(const Ctx &c) {
    size_t blocks = ((size_t)c.np + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    return dim3((unsigned)blocks);
}

void launch_axpy(Ctx &c, double a, const double *x, double *y) {
    hipLaunchKernelGGL(axpy_kernel, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, a, x, y);
}
// y = x / sqrt(d_red[slot]) (0 when that norm is 0 or not finite): normalisation without a host
// round trip
__global__ void normalise_copy_kernel(size_t n, const double *__restrict__ red, int slot,
                                      const double *__restrict__ x, double *__restrict__ y) {
    const double n2 = red[slot];
    const double a = (n2 > 0.0 && n2 < 1.7e308) ? 1.0 / sqrt(n2) : 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = a * x[i];
}

void launch_normalise_copy(Ctx &c, int slot, const double *x, double *y) {
    hipLaunchKernelGGL(normalise_copy_kernel, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, c.d_red, slot,
                       x, y);
}

void launch_scale_copy(Ctx &c, double a, const double *x, double *y) {
    hipLaunchKernelGGL(scale_copy_kernel, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, a, x, y);
}

struct CoefPack8 {
    double c[8];
};

template <int K>
__global__ void multi_axpy_kernel(size_t n, CoefPack8 cf, PtrPack8 xs, double *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double s = y[i];
#pragma unroll
        for (int k = 0; k < K; ++k) s += cf.c[k] * xs.p[k][i];
        y[i] = s;
    }
}

void launch_multi_axpy(Ctx &c, const double *coef_host, int k, const double *const *xs, double *y, double sign) {
    int done = 0;
    while (done < k) {
        const int kk = (k - done) >= 8 ? 8 : (k - done);
        PtrPack8 pk;
        CoefPack8 cf;
        for (int i = 0; i < 8; ++i) {
            pk.p[i] = xs[done + (i < kk ? i : 0)];
            cf.c[i] = i < kk ? sign * coef_host[done + i] : 0.0;
        }
        switch (kk) {
            case 1: hipLaunchKernelGGL(multi_axpy_kernel<1>, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, cf, pk, y); break;
            case 2: hipLaunchKernelGGL(multi_axpy_kernel<2>, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, cf, pk, y); break;
            case 3: hipLaunchKernelGGL(multi_axpy_kernel<3>, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, cf, pk, y); break;
            case 4: hipLaunchKernelGGL(multi_axpy_kernel<4>, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, cf, pk, y); break;
            case 5: hipLaunchKernelGGL(multi_axpy_kernel<5>, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, cf, pk, y); break;
            case 6: hipLaunchKernelGGL(multi_axpy_kernel<6>, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, cf, pk, y); break;
            case 7: hipLaunchKernelGGL(multi_axpy_kernel<7>, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, cf, pk, y); break;
            default: hipLaunchKernelGGL(multi_axpy_kernel<8>, vec_grid(c), dim3(256), 0, c.stream, (size_t)c.np, cf, pk, y); break;
        }
        done += kk;
    }
}

// Newton update in one pass: delta = sum_i c_i z_i, u += delta, and the per-block partial sums of
// |delta|^2 and |u|^2 over the owned entries (slots 1, 2 of the reduction buffer) -- instead of a
// memset, a multi-axpy, an axpy and two norm kernels.
template <int K>
__global__ __launch_bounds__(256) void newton_update_kernel(size_t n, size_t n_dot, CoefPack8 cf, PtrPack8 zs,
                                                            double *__restrict__ u, double *__restrict__ delta,
                                                            double *__restrict__ partials) {
    double acc[2] = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) d += cf.c[k] * zs.p[k][i];
        const double un = u[i] + d;
        u[i] = un;
        if (delta) delta[i] = d;   // (nobody reads it after a solve that converged in its first cycle)
        if (i < n_dot) {
            acc[0] += d * d;
            acc[1] += un * un;
        }
    }
    block_reduce_store<2>(acc, partials, 1);
}

__global__ void reduce_partials_range_kernel(const double *__restrict__ partials, int nblocks, int k0,
                                             double *__restrict__ out) {
    const int i = k0 + blockIdx.x;  // one wave per output; fixed summation order
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) s += partials[PARTIAL_AT(b, i)];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[i] = s;
}

void launch_newton_update(Ctx &c, const double *coef_host, int k, const double *const *zs, double *u,
                          double *delta) {
    const int grid = red_grid(c);
    PtrPack8 pk;
    CoefPack8 cf;
    for (int i = 0; i < 8; ++i) {
        pk.p[i] = zs[i < k ? i : 0];
        cf.c[i] = i < k ? coef_host[i] : 0.0;
    }
#define FEDM_NU(K)                                                                                         \
    hipLaunchKernelGGL(newton_update_kernel<K>, dim3(grid), dim3(256), 0, c.stream, (size_t)c.np, (size_t)c.n_dot, \
                       cf, pk, u, delta, c.d_partials)
    switch (k) {
        case 1: FEDM_NU(1); break;
        case 2: FEDM_NU(2); break;
        case 3: FEDM_NU(3); break;
        case 4: FEDM_NU(4); break;
        case 5: FEDM_NU(5); break;
        case 6: FEDM_NU(6); break;
        case 7: FEDM_NU(7); break;
        default: FEDM_NU(8); break;
    }
#undef FEDM_NU
    hipLaunchKernelGGL(reduce_partials_range_kernel, dim3(2), dim3(64), 0, c.stream, c.d_partials, grid, 1, c.d_red);
    // several GPUs: d_red[1], d_red[2] stay rank-local; they are all-reduced together with the next |F|^2
    // (norm2_publish, k_sum = 3): Ctx::red12_local tells the Newton loop
    c.red12_local = c.comm != nullptr;
}

// |new - old + eps|^2 and |old + eps|^2 over one component (fedm/functions.py:1062-1064)
__global__ __launch_bounds__(256) void field_error_kernel(int nv, int neq, int comp,
                                                          const double *__restrict__ u,
                                                          const double *__restrict__ uold,
                                                          double *__restrict__ partials, int slot0) {
    const double eps = 3.0e-16;  // DOLFIN_EPS
    double acc[2] = {0.0, 0.0};
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += gridDim.x * blockDim.x) {
        const double a = u[(size_t)v * neq + comp], b = uold[(size_t)v * neq + comp];
        const double d = a - b + eps, o = b + eps;
        acc[0] += d * d;
        acc[1] += o * o;
    }
    block_reduce_store<2>(acc, partials, slot0);
}

void launch_field_error(Ctx &c, int comp) {
    int grid = (c.n_owned + 255) / 256;
    if (grid > RED_BLOCKS) grid = RED_BLOCKS;
    hipLaunchKernelGGL(field_error_kernel, dim3(grid), dim3(256), 0, c.stream, c.n_owned, c.neq, comp, c.d_u, c.d_uold, c.d_partials, 0);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(2), dim3(64), 0, c.stream, c.d_partials, grid, 2, c.d_red);
    comm_allreduce(c, c.d_red, 2);
}

// the same two sums into d_red[3], d_red[4]: they ride on the next publication (several GPUs: rank-local
// until norm2_publish all-reduces them with |F|^2)
void launch_field_error_slots34(Ctx &c, int comp) {
    int grid = (c.n_owned + 255) / 256;
    if (grid > RED_BLOCKS) grid = RED_BLOCKS;
    hipLaunchKernelGGL(field_error_kernel, dim3(grid), dim3(256), 0, c.stream, c.n_owned, c.neq, comp, c.d_u, c.d_uold, c.d_partials, 3);
    hipLaunchKernelGGL(reduce_partials_range_kernel, dim3(2), dim3(64), 0, c.stream, c.d_partials, grid, 3, c.d_red);
}

// =============================================================================================
// Copy ceiling of the box: 16-byte-per-lane copies (what MI355X_MICROARCH.md measures 6.29 TB/s
// with), read + write bytes over HIP-event time.  Buffers far beyond the 256 MiB Infinity Cache;
// bench.py prints the rate next to the 8 TB/s specification.  A ceiling has to be the best a copy
// reaches on the box, so several shapes are timed and the fastest one is reported: U loads in
// flight per lane before the first store (round 3's single load per trip left the memory system
// half empty: 4.8 TB/s, below what the Jacobian product moves), plain or non-temporal.
// =============================================================================================
typedef float copy_f4 __attribute__((ext_vector_type(4)));   // (the non-temporal builtins take native vectors)
template <int U, bool NT>
__global__ __launch_bounds__(256) void copy16_kernel(const copy_f4 *__restrict__ src, copy_f4 *__restrict__ dst, size_t n) {
    // a workgroup takes contiguous chunks of U * 256 pieces; the grid strides over the chunks
    const size_t chunk = (size_t)U * 256;
    for (size_t base = (size_t)blockIdx.x * chunk; base < n; base += (size_t)gridDim.x * chunk) {
        copy_f4 v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const size_t i = base + (size_t)k * 256 + threadIdx.x;
            if (i < n) {
                if (NT) v[k] = __builtin_nontemporal_load(src + i);
                else v[k] = src[i];
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const size_t i = base + (size_t)k * 256 + threadIdx.x;
            if (i < n) {
                if (NT) __builtin_nontemporal_store(v[k], dst + i);
                else dst[i] = v[k];
            }
        }
    }
}

int copy_bandwidth(int device, int64_t bytes, int repeats, double *gbs) {
    FEDM_HIP_CHECK(hipSetDevice(device));
    const size_t n = (size_t)bytes / sizeof(copy_f4);
    copy_f4 *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = -1;
    do {
        if (hipMalloc((void **)&a, n * sizeof(copy_f4)) != hipSuccess) break;
        if (hipMalloc((void **)&b, n * sizeof(copy_f4)) != hipSuccess) break;
        if (hipMemset(a, 1, n * sizeof(copy_f4)) != hipSuccess) break;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) break;
        double best = 0.0;
        bool failed = false;
        for (int variant = 0; variant < 6 && !failed; ++variant) {
            // grids: as many workgroups as there are chunks, up to 16 per CU (256 CUs)
            static const int unroll_of[6] = {1, 4, 4, 8, 8, 2};
            const size_t per = (size_t)unroll_of[variant] * 256;
            const unsigned g = (unsigned)std::min<size_t>((n + per - 1) / per, (size_t)256 * 16);
            auto launch = [&]() {
                switch (variant) {
                    case 0: hipLaunchKernelGGL((copy16_kernel<1, false>), dim3(256 * 8), dim3(256), 0, 0, a, b, n); break;
                    case 1: hipLaunchKernelGGL((copy16_kernel<4, false>), dim3(g), dim3(256), 0, 0, a, b, n); break;
                    case 2: hipLaunchKernelGGL((copy16_kernel<4, true>), dim3(g), dim3(256), 0, 0, a, b, n); break;
                    case 3: hipLaunchKernelGGL((copy16_kernel<8, false>), dim3(g), dim3(256), 0, 0, a, b, n); break;
                    case 4: hipLaunchKernelGGL((copy16_kernel<8, true>), dim3(g), dim3(256), 0, 0, a, b, n); break;
                    default: hipLaunchKernelGGL((copy16_kernel<2, false>), dim3(g), dim3(256), 0, 0, a, b, n); break;
                }
            };
            launch();
            if (hipDeviceSynchronize() != hipSuccess) { failed = true; break; }
            hipEventRecord(e0, 0);
            for (int i = 0; i < repeats; ++i) launch();
            hipEventRecord(e1, 0);
            if (hipEventSynchronize(e1) != hipSuccess) { failed = true; break; }
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            const double rate = 2.0 * (double)(n * sizeof(copy_f4)) * repeats / ((double)ms * 1e-3) / 1e9;
            if (std::getenv("FEDM_COPY_VERBOSE")) fprintf(stderr, "copy_bandwidth variant %d: %.0f GB/s\n", variant, rate);
            best = std::max(best, rate);
        }
        if (failed) break;
        *gbs = best;
        rc = 0;
    } while (false);
    if (rc) set_error("copy_bandwidth: HIP call failed (out of memory?)");
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (a) hipFree(a);
    if (b) hipFree(b);
    return rc;
}

}  // namespace fedm
