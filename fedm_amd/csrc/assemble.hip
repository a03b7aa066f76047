// Volume assembly of the FEDM hot path (gfx950, fp64, no MFMA): the coloured, the LDS-patch and the row-phase (lean2)
// element assembly into the sliced block-ELL Jacobian with the host decision between them and the one-pass kernels of
// assemble3.hip (assembly_path).  What follows the volume kernel -- the boundary facets, the Dirichlet and identity
// rows -- is boundary.hip.
#include <cstdlib>

#include "comm.hpp"
#include "device_util.hpp"
#include "dielectric.hpp"
#include "element.hpp"
#include "element_lean.hpp"
#include "fedm_internal.hpp"

namespace fedm {

// The ghost entries of the state are refreshed lazily: the Newton loop only marks them stale
// (Ctx::halo_pending) and the next assembly either overlaps the exchange with its interior
// patches or, on every other path, performs it here first.
static void flush_pending_halo(Ctx &c) {
    if (!c.halo_pending) return;
    comm_halo(c, c.d_u);
    c.halo_pending = false;
}

// =============================================================================================
// Assembly, variant 0: one thread per cell, one launch per colour (cells of a colour share
// no vertex, so the read-modify-write of matrix blocks and residual entries is conflict-free
// and the summation order is fixed -> bitwise reproducible).
// Problem.F / Problem.J, fedm/functions.py:188-202
// =============================================================================================
template <int NS, bool PO, int NR, int CACHE, bool LIN, bool TAB>
__global__ __launch_bounds__(256) void assemble_colour_kernel(
    const fedm_model_desc *__restrict__ md, const int *__restrict__ cell_list, int n_cells,
    const int *__restrict__ cells, const double *__restrict__ coords,
    const uint32_t *__restrict__ cell_slots, const double *__restrict__ u,
    const double *__restrict__ uold, const double *__restrict__ uold1, StepCoef sc,
    const double *ext0, const double *ext1, const double *ext2, const double *ext3,
    double *__restrict__ val, double *__restrict__ F, int jacobian, int mode) {
    constexpr int NEQ = NS + (PO ? 1 : 0);
    constexpr int NEQ2 = NEQ * NEQ;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cells) return;
    const int c = cell_list[t];
    int v[3];
    double x[3][2], Uc[3][NEQ], Hc[3][NS];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v[a] = cells[3 * c + a];
        x[a][0] = coords[2 * v[a]];
        x[a][1] = coords[2 * v[a] + 1];
#pragma unroll
        for (int s = 0; s < NEQ; ++s) Uc[a][s] = u[(size_t)v[a] * NEQ + s];
#pragma unroll
        for (int s = 0; s < NS; ++s)
            Hc[a][s] = sc.c_old * uold[(size_t)v[a] * NEQ + s] + sc.c_old1 * uold1[(size_t)v[a] * NEQ + s];
    }
    const double *extp[4] = {ext0, ext1, ext2, ext3};
    const double *ext[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
        ext[s] = (extp[s] && md->ext_nodes[s]) ? extp[s] + (size_t)c * md->ext_nodes[s] : nullptr;

    Element<NS, PO, NR, CACHE, LIN, TAB> el;
    el.setup(md, x, Uc, Hc, sc, mode);
    uint32_t slot[9];
    if (jacobian) {
#pragma unroll
        for (int k = 0; k < 9; ++k) slot[k] = cell_slots[(size_t)c * 9 + k];
    }
#pragma unroll
    for (int row = 0; row < NEQ; ++row) {
        if (mode == 1 && PO && row != NEQ - 1) continue;  // Poisson-only: species rows are identity
        el.row_moments(md, row, Uc, Hc, sc, ext);
            el.row_prepare(md, row);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            F[(size_t)v[a] * NEQ + row] += el.residual(row, a);
            if (!jacobian) continue;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                double B[NEQ];
                el.block_row(md, row, a, b, B);
                const uint32_t sl = slot[a * 3 + b];
                double *dst = val + ((size_t)(sl >> 6) * NEQ2 + row * NEQ) * SLICE + (sl & 63);
#pragma unroll
                for (int i = 0; i < NEQ; ++i) dst[(size_t)i * SLICE] += B[i];
            }
        }
    }
}

template <int NS, bool PO, int NR, int CACHE, bool LIN, bool TAB>
static void assemble_colour_t(Ctx &c, bool jacobian, int mode) {
    constexpr int NEQ = NS + (PO ? 1 : 0);
    flush_pending_halo(c);
    hipMemsetAsync(c.d_F, 0, sizeof(double) * c.np, c.stream);
    if (jacobian)
        hipMemsetAsync(c.d_val, 0, sizeof(double) * (size_t)c.pat.total_bc * SLICE * NEQ * NEQ, c.stream);
    const StepCoef sc = step_coef(c.dt, c.dt_old);
    const int ncol = (int)c.pat.colour_ptr.size() - 1;
    for (int k = 0; k < ncol; ++k) {
        const int n = c.pat.colour_ptr[k + 1] - c.pat.colour_ptr[k];
        if (n == 0) continue;
        hipLaunchKernelGGL((assemble_colour_kernel<NS, PO, NR, CACHE, LIN, TAB>), dim3((n + 255) / 256), dim3(256), 0,
                           c.stream, c.d_model, c.d_colour_cells + c.pat.colour_ptr[k], n,
                           c.d_cells, c.d_coords, c.d_cell_slots, c.d_u, c.d_uold, c.d_uold1, sc,
                           c.d_ext[0], c.d_ext[1], c.d_ext[2], c.d_ext[3], c.d_val, c.d_F,
                           jacobian ? 1 : 0, mode);
        note_assembly_launch(c, jacobian, 0, 256, (n + 255) / 256);
    }
}

// =============================================================================================
// Assembly, variant 1 (default): LDS patches.  One workgroup owns one matrix slice (64 vertex
// rows).  It stages the patch's vertex data (owned + halo vertices: coordinates, u and the
// folded BDF history) in LDS, evaluates every cell that touches an owned vertex (cells on
// patch borders are evaluated by each patch they touch), accumulates the owned rows' blocks
// and residual entries in LDS with ds_add_f64, and finally streams the finished slice out
// with fully coalesced stores: every matrix value is written exactly once -- no
// read-modify-write in HBM and no zero-fill pass.
// =============================================================================================

#ifdef FEDM_PHASE_TIMING
__device__ unsigned long long g_phase[8];
#define FEDM_T(k) if (threadIdx.x == 0) { const unsigned long long now_ = wall_clock64(); atomicAdd(&g_phase[k], now_ - t_prev_); t_prev_ = now_; }
extern "C" void fedm_debug_phase(unsigned long long *out, int reset) {
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 8);
    if (reset) {
        unsigned long long z[8] = {0};
        hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z));
    }
}
#else
#define FEDM_T(k)
#endif

// The kernel sits at 237-255 VGPRs; amdgpu_waves_per_eu pins it to two waves per SIMD (one
// wave per SIMD is 1.5x slower) should a compiler change push it over 256.
// THREADS: workgroup size = the patch's cell count rounded up (192 for Z-ordered meshes: two
// 3-wave workgroups per CU at 2 waves/SIMD keep 6 waves busy; 320 covers 1-D strips)
// JAC = false is the residual-only assembly (final Newton check): without the Jacobian code it
// needs about half the registers and no accumulators, so it is compiled as a kernel of its own
// that the compiler may run at a higher occupancy.
template <int NS, bool PO, int NR, int CACHE, int THREADS, bool JAC, bool LIN, bool TAB>
__device__ __forceinline__ void assemble_patch_body(
    const fedm_model_desc *__restrict__ md, int nv, const int *__restrict__ boff,
    const int *__restrict__ cell_ptr, const PatchCell *__restrict__ pcells,
    const int *__restrict__ halo_ptr, const int *__restrict__ halo,
    const double *__restrict__ coords, const double *__restrict__ u,
    const double *__restrict__ uold, const double *__restrict__ uold1, StepCoef sc,
    const double *ext0, const double *ext1, const double *ext2, const double *ext3,
    double *__restrict__ val, double *__restrict__ F, int mode, int acc_doubles,
    int max_verts) {
    constexpr bool jacobian = JAC;
    constexpr int NEQ = NS + (PO ? 1 : 0);
    constexpr int NEQ2 = NEQ * NEQ;
    extern __shared__ __align__(16) double lds[];
    double *acc = lds;                          // [width][NEQ2][64]
    double *Fl = acc + acc_doubles;             // [64][NEQ]
    double *vx = Fl + SLICE * NEQ;              // [max_verts][2]
    double *Ul = vx + 2 * max_verts;            // [max_verts][NEQ]
    double *Hl = Ul + NEQ * max_verts;          // [max_verts][NS]

#ifdef FEDM_PHASE_TIMING
    unsigned long long t_prev_ = wall_clock64();
#endif
    const int S = blockIdx.x;
    const int b0 = boff[S], width = boff[S + 1] - b0;
    const int n_acc = jacobian ? width * NEQ2 * SLICE : 0;  // a multiple of 64: 16-byte LDS / HBM accesses
    {
        double2 *acc2 = reinterpret_cast<double2 *>(acc);
        for (int k = threadIdx.x; k < n_acc / 2; k += blockDim.x) acc2[k] = make_double2(0.0, 0.0);
    }
    for (int k = threadIdx.x; k < SLICE * NEQ; k += blockDim.x) Fl[k] = 0.0;
    FEDM_T(0)
    const int h0 = halo_ptr[S], n_local = SLICE + halo_ptr[S + 1] - h0;
    for (int i = threadIdx.x; i < n_local; i += blockDim.x) {
        const int g = (i < SLICE) ? S * SLICE + i : halo[h0 + i - SLICE];
        if (g < nv) {
            vx[2 * i] = coords[2 * (size_t)g];
            vx[2 * i + 1] = coords[2 * (size_t)g + 1];
#pragma unroll
            for (int s = 0; s < NEQ; ++s) Ul[i * NEQ + s] = u[(size_t)g * NEQ + s];
#pragma unroll
            for (int s = 0; s < NS; ++s)
                Hl[i * NS + s] = sc.c_old * uold[(size_t)g * NEQ + s] + sc.c_old1 * uold1[(size_t)g * NEQ + s];
        }
    }
    FEDM_T(1)
    __syncthreads();
    FEDM_T(2)

    const int c0 = cell_ptr[S], n_cells = cell_ptr[S + 1] - c0;
    for (int i = threadIdx.x; i < n_cells; i += blockDim.x) {
        const PatchCell pc = pcells[c0 + i];
        double x[3][2], Uc[3][NEQ], Hc[3][NS];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int l = pc.lv[a];
            x[a][0] = vx[2 * l];
            x[a][1] = vx[2 * l + 1];
#pragma unroll
            for (int s = 0; s < NEQ; ++s) Uc[a][s] = Ul[l * NEQ + s];
#pragma unroll
            for (int s = 0; s < NS; ++s) Hc[a][s] = Hl[l * NS + s];
        }
        const double *extp[4] = {ext0, ext1, ext2, ext3};
        const double *ext[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s)
            ext[s] = (extp[s] && md->ext_nodes[s]) ? extp[s] + (size_t)pc.cell * md->ext_nodes[s] : nullptr;

        FEDM_T(3)
        Element<NS, PO, NR, CACHE, LIN, TAB> el;
        el.setup(md, x, Uc, Hc, sc, mode);
        FEDM_T(4)
#pragma unroll
        for (int row = 0; row < NEQ; ++row) {
            if (mode == 1 && PO && row != NEQ - 1) continue;
            el.row_moments(md, row, Uc, Hc, sc, ext);
            el.row_prepare(md, row);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int lane = pc.lv[a];
                if (lane >= SLICE) continue;  // row vertex owned by another patch
                unsafeAtomicAdd(&Fl[lane * NEQ + row], el.residual(row, a));
                if (!jacobian) continue;
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    double B[NEQ];
                    el.block_row(md, row, a, b, B);
                    double *dst = acc + ((size_t)pc.j[a * 3 + b] * NEQ2 + row * NEQ) * SLICE + lane;
#pragma unroll
                    for (int i = 0; i < NEQ; ++i) unsafeAtomicAdd(&dst[i * SLICE], B[i]);
                }
            }
        }
    }
    FEDM_T(5)
    __syncthreads();
    FEDM_T(6)
    {
        double2 *vdst2 = reinterpret_cast<double2 *>(val + (size_t)b0 * NEQ2 * SLICE);
        const double2 *acc2 = reinterpret_cast<const double2 *>(acc);
        for (int k = threadIdx.x; k < n_acc / 2; k += blockDim.x) vdst2[k] = acc2[k];
    }
    double *fdst = F + (size_t)S * SLICE * NEQ;
    for (int k = threadIdx.x; k < SLICE * NEQ; k += blockDim.x) fdst[k] = Fl[k];
    FEDM_T(7)
}

#define FEDM_PATCH_PARAMS                                                                          \
    const fedm_model_desc *__restrict__ md, int nv, const int *__restrict__ boff,                  \
        const int *__restrict__ cell_ptr, const PatchCell *__restrict__ pcells,                    \
        const int *__restrict__ halo_ptr, const int *__restrict__ halo,                            \
        const double *__restrict__ coords, const double *__restrict__ u,                           \
        const double *__restrict__ uold, const double *__restrict__ uold1, StepCoef sc,            \
        const double *ext0, const double *ext1, const double *ext2, const double *ext3,            \
        double *__restrict__ val, double *__restrict__ F, int mode, int acc_doubles, int max_verts
#define FEDM_PATCH_ARGS                                                                            \
    md, nv, boff, cell_ptr, pcells, halo_ptr, halo, coords, u, uold, uold1, sc, ext0, ext1, ext2,  \
        ext3, val, F, mode, acc_doubles, max_verts

template <int NS, bool PO, int NR, int CACHE, int THREADS, bool LIN, bool TAB>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void assemble_patch_kernel(
    FEDM_PATCH_PARAMS) {
    assemble_patch_body<NS, PO, NR, CACHE, THREADS, true, LIN, TAB>(FEDM_PATCH_ARGS);
}

template <int NS, bool PO, int NR, int CACHE, int THREADS, bool LIN, bool TAB>
__global__ __launch_bounds__(THREADS) void residual_patch_kernel(FEDM_PATCH_PARAMS) {
    assemble_patch_body<NS, PO, NR, CACHE, THREADS, false, LIN, TAB>(FEDM_PATCH_ARGS);
}

// workgroup barrier that orders LDS accesses only: global stores issued before it stay in flight
__device__ __forceinline__ void lds_only_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Second generation of the row-phase kernel (element_lean.hpp, lean2_*): per-vertex exponentials,
// cell constants kept in an LDS column between the rows; JAC = false is the residual-only assembly.
template <int NS, int NR, int THREADS, bool JAC, bool TAB>
__device__ __forceinline__ void assemble_lean2_body(FEDM_PATCH_PARAMS, int xcd, const int *__restrict__ patch_list,
                                                    uint32_t cmask) {
    constexpr int NEQ = NS + 1, NEQ2 = NEQ * NEQ;
    constexpr int NST = LeanStash<NR>::N;
    extern __shared__ __align__(16) double lds[];
    double *acc = lds;                          // [width][NEQ][64]: one row of every block (JAC)
    double *Fl = acc + acc_doubles;             // [64][NEQ]
    double *vx = Fl + SLICE * NEQ;              // [max_verts][2]
    double *Ul = vx + 2 * max_verts;            // [max_verts][NEQ]
    double *Hl = Ul + NEQ * max_verts;          // [max_verts][NS]
    double *Al = Hl + NS * max_verts;           // [max_verts][NS]: exp(u / 6)
    double *cst = Al + NS * max_verts;          // [NST][THREADS]
#ifdef FEDM_PHASE_TIMING
    unsigned long long t_prev_ = wall_clock64();
#endif
    // patch_list: the launch covers those patches only (interior / boundary halves across GPUs)
    const int blk = xcd ? xcd_contiguous(blockIdx.x, gridDim.x) : blockIdx.x;
    const int S = patch_list ? patch_list[blk] : blk;
    const int b0 = boff[S], width = boff[S + 1] - b0;
    const int n_acc = JAC ? width * NEQ * SLICE : 0;
    const int c0 = cell_ptr[S], n_cells = cell_ptr[S + 1] - c0;
    const bool active = (int)threadIdx.x < n_cells;   // one cell per thread (n_cells <= THREADS)
    PatchCell pc_own = {};
    if (active) pc_own = pcells[c0 + threadIdx.x];
    if constexpr (JAC) {
        double2 *acc2 = reinterpret_cast<double2 *>(acc);
        for (int k = threadIdx.x; k < n_acc / 2; k += THREADS) acc2[k] = make_double2(0.0, 0.0);
    }
    for (int k = threadIdx.x; k < SLICE * NEQ; k += THREADS) Fl[k] = 0.0;
    const int h0 = halo_ptr[S], n_local = SLICE + halo_ptr[S + 1] - h0;
    for (int i = threadIdx.x; i < n_local; i += THREADS) {
        const int g = (i < SLICE) ? S * SLICE + i : halo[h0 + i - SLICE];
        if (g < nv) {
            vx[2 * i] = coords[2 * (size_t)g];
            vx[2 * i + 1] = coords[2 * (size_t)g + 1];
            double un[NEQ];
#pragma unroll
            for (int s = 0; s < NEQ; ++s) un[s] = u[(size_t)g * NEQ + s];
#pragma unroll
            for (int s = 0; s < NS; ++s)
                Hl[i * NS + s] = sc.c_old * uold[(size_t)g * NEQ + s] + sc.c_old1 * uold1[(size_t)g * NEQ + s];
#pragma unroll
            for (int s = 0; s < NEQ; ++s) Ul[i * NEQ + s] = un[s];
#pragma unroll
            for (int s = 0; s < NS; ++s) Al[i * NS + s] = exp(un[s] * (1.0 / 6.0));
        }
    }
    FEDM_T(0)   // zero + stage (issue) + vertex exponentials
    __syncthreads();
    FEDM_T(1)   // barrier: the staged loads arrive
    LeanCell lc = {0, 0, 0, 0};
    if (active) lc = lean2_prologue<NS, NR, TAB>(md, pc_own, vx, Ul, cst + threadIdx.x, THREADS);
    FEDM_T(2)   // prologue: cell record, field, rate coefficient
    if constexpr (!JAC) {
        // residual only: no accumulators, no row phases -- the rows share the cell's geometry
        if (active) {
            int lv[3];
            double G[3][2], W[3];
            lean2_geometry(md, lc, vx, lv, G, W, cst[LeanStash<NR>::IDET * THREADS + threadIdx.x]);
#pragma unroll
            for (int row = 0; row < NEQ; ++row)
                lean2_row_core<NS, NR, false, -1, TAB>(md, row, lc, lv, G, W, Ul, Hl, Al, sc, acc, Fl, cst + threadIdx.x, THREADS);
        }
    }
#pragma unroll 1
    for (int row = 0; JAC && row < NEQ; ++row) {
        asm volatile("" : "+v"(lc.wl), "+v"(lc.wj0), "+v"(lc.wj1), "+v"(lc.wj2));  // nothing hoisted out of the row
        if (active) {
#ifndef FEDM_LEAN2_ROW_GENERIC
            // one body per equation row: the row index is a compile-time constant inside each (the
            // selects on it fold away: 161 -> 144 VGPRs, -3 %; -DFEDM_LEAN2_ROW_GENERIC: one shared body)
#define FEDM_ROW_CASE(R)                                                                                   \
    case R:                                                                                                \
        if constexpr (NEQ > R)                                                                             \
            lean2_row<NS, NR, JAC, R, TAB>(md, row, lc, vx, Ul, Hl, Al, sc, acc, Fl, cst + threadIdx.x, THREADS, cmask); \
        break;
            switch (row) {
                FEDM_ROW_CASE(0)
                FEDM_ROW_CASE(1)
                FEDM_ROW_CASE(2)
                FEDM_ROW_CASE(3)
                FEDM_ROW_CASE(4)
            }
#undef FEDM_ROW_CASE
#else
            lean2_row<NS, NR, JAC, -1, TAB>(md, row, lc, vx, Ul, Hl, Al, sc, acc, Fl, cst + threadIdx.x, THREADS, cmask);
#endif
        }
        FEDM_T(3)   // the row (wave 0's view)
        if constexpr (JAC) {
            __syncthreads();
            FEDM_T(4)   // barrier: the other waves finish the row
            constexpr int PER = NEQ * SLICE / 2;   // 16-byte pieces per block column
            // planes that never change (cmask) are neither read out nor zeroed: 32 pieces per plane
            const uint32_t rmask = cmask >> (row * NEQ);
            if constexpr (THREADS % PER == 0) {
                // a thread keeps its place within the block column and strides over the columns: all
                // its LDS reads are issued before the first store waits for one of them
                int tid = threadIdx.x;
                asm volatile("" : "+v"(tid));   // keeps the addresses below out of the row loop's live state
                const int rem = tid % PER;
                constexpr int STEP = THREADS / PER;
                double2 *srcs = reinterpret_cast<double2 *>(acc) + rem;
                if (!((rmask >> (rem / (SLICE / 2))) & 1u)) {
                    // two block columns per pass: both LDS reads are in flight before the first store
                    int bc = tid / PER;
                    for (; bc + STEP < width; bc += 2 * STEP) {
                        const double2 a = srcs[bc * PER], b = srcs[(bc + STEP) * PER];
                        reinterpret_cast<double2 *>(val + ((size_t)(b0 + bc) * NEQ2 + row * NEQ) * SLICE)[rem] = a;
                        reinterpret_cast<double2 *>(val + ((size_t)(b0 + bc + STEP) * NEQ2 + row * NEQ) * SLICE)[rem] = b;
                        srcs[bc * PER] = make_double2(0.0, 0.0);
                        srcs[(bc + STEP) * PER] = make_double2(0.0, 0.0);
                    }
                    if (bc < width) {
                        reinterpret_cast<double2 *>(val + ((size_t)(b0 + bc) * NEQ2 + row * NEQ) * SLICE)[rem] = srcs[bc * PER];
                        srcs[bc * PER] = make_double2(0.0, 0.0);
                    }
                }
            } else {
                for (int k = threadIdx.x; k < n_acc / 2; k += THREADS) {
                    const int bc = k / PER, rem = k - bc * PER;
                    if ((rmask >> (rem / (SLICE / 2))) & 1u) continue;
                    double2 *dst = reinterpret_cast<double2 *>(val + ((size_t)(b0 + bc) * NEQ2 + row * NEQ) * SLICE);
                    double2 *src = reinterpret_cast<double2 *>(acc) + k;
                    dst[rem] = *src;
                    *src = make_double2(0.0, 0.0);
                }
            }
            FEDM_T(5)   // stream-out + zeroing (issue)
            lds_only_barrier();   // accumulators zero again; the stores above stay in flight
            FEDM_T(6)
        }
    }
    if constexpr (!JAC) __syncthreads();
    double *fdst = F + (size_t)S * SLICE * NEQ;
    for (int k = threadIdx.x; k < SLICE * NEQ; k += THREADS) fdst[k] = Fl[k];
    FEDM_T(7)
}

#ifndef FEDM_LEAN2_WAVES
#define FEDM_LEAN2_WAVES 3
#endif
template <int NS, int NR, int THREADS, bool TAB>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(FEDM_LEAN2_WAVES, FEDM_LEAN2_WAVES))) void assemble_lean2_kernel(
    FEDM_PATCH_PARAMS, int xcd, const int *__restrict__ patch_list, uint32_t cmask) {
    assemble_lean2_body<NS, NR, THREADS, true, TAB>(FEDM_PATCH_ARGS, xcd, patch_list, cmask);
}

template <int NS, int NR, int THREADS, bool TAB>
__global__ __launch_bounds__(THREADS) void residual_lean2_kernel(FEDM_PATCH_PARAMS, int xcd,
                                                                 const int *__restrict__ patch_list, uint32_t cmask) {
    assemble_lean2_body<NS, NR, THREADS, false, TAB>(FEDM_PATCH_ARGS, xcd, patch_list, cmask);
}
#undef FEDM_PATCH_PARAMS
#undef FEDM_PATCH_ARGS

size_t patch_lds_bytes(const Ctx &c, bool jacobian) {
    const int neq = c.neq, mv = c.pat.max_patch_verts;
    const size_t acc = jacobian ? (size_t)c.pat.max_patch_width * neq * neq * SLICE : 0;
    return sizeof(double) * (acc + SLICE * neq + 2 * mv + (size_t)(neq + c.ns) * mv);
}

// ... of the row-phase kernels (assemble_lean2_body's arrays): one row of every block, the vertex exponentials besides,
// and `n_stash` cell constants (LeanStash<NR>::N) for each of the workgroup's threads
static size_t lean2_lds_bytes(const Ctx &c, bool jacobian, int n_stash, int threads) {
    const int neq = c.neq, mv = c.pat.max_patch_verts;
    const size_t acc_row = jacobian ? (size_t)c.pat.max_patch_width * neq * SLICE : 0;
    return sizeof(double) * (acc_row + SLICE * neq + 2 * mv + (size_t)(neq + 2 * c.ns) * mv + (size_t)n_stash * threads);
}

// LDS patch assembly can run on this mesh and model at all (else the global colouring: context creation and
// fedm_set_assembly): 8-bit local indices, the generic kernel's LDS within a workgroup's 160 KiB, the LFA family.
bool patch_assembly_available(const Ctx &c) {
    return c.pat.patch_ok && patch_lds_bytes(c) <= WORKGROUP_LDS_BYTES && c.model_kind != 1;
}

// FIAT's degree-2 rule (points (1/6,1/6), (1/6,2/3), (2/3,1/6), weights 1/6): the kernels take it as constants
static bool fiat_degree2_rule(const fedm_model_desc &m) {
    const double sixth = 1.0 / 6.0, two3 = 2.0 / 3.0;
    return m.n_qp == 3 && m.qp_x[0] == sixth && m.qp_x[1] == sixth && m.qp_x[2] == two3 && m.qp_y[0] == sixth &&
           m.qp_y[1] == two3 && m.qp_y[2] == sixth && m.qp_w[0] == sixth && m.qp_w[1] == sixth && m.qp_w[2] == sixth;
}

// some species has an external source
static bool has_ext_source(const Ctx &c) {
    bool ext = false;
    for (int s = 0; s < c.ns; ++s) ext = ext || c.model.ext_nodes[s] > 0;
    return ext;
}

// The models the row-phase and one-pass kernels exist for: the template instance assemble_dispatch takes for the LFA
// family with Poisson, FIAT's degree-2 rule and the logarithmic representation (PO && CACHE == 2 && !LIN), with no
// external source and FEDM_ASSEMBLY_LEAN at 2 or above (the one-pass kernels besides: lean3_applies).
// (one predicate for assembly_path and launch_assemble_species)
static bool lean_model_applies(const Ctx &c) {
    return c.model_kind == 0 && c.poisson && c.ns >= 1 && c.ns <= 4 && !c.model.linear_representation &&
           fiat_degree2_rule(c.model) && !has_ext_source(c) && c.assembly_lean >= 2;
}

// The volume kernel an assembly of this context as it stands takes (AssemblyPath, fedm_internal.hpp) -- the only place
// that decides it: launch_assemble launches what this returns, fedm_pattern_info reports it for mode 0.
// max_variant = 2 strikes the third generation out (what is left when its launch fails).
static AssemblyPath assembly_path_upto(const Ctx &c, bool jacobian, int mode, int max_variant) {
    if (c.model_kind != 0) return {-1, 0, 0u};
    if (c.assembly_kind == 0) return {0, 256, 0u};
    const int cells = c.pat.max_patch_cells;
    if (mode == 0 && lean_model_applies(c)) {
        // the constant potential-potential plane: written by the first full assembly, kept afterwards
        const uint32_t cmask = (jacobian && c.skip_const_planes && c.const_planes_valid) ? c.const_plane_mask : 0u;
        // The third generation takes patches of up to 384 cells (a second cell for some threads) where its LDS fits
        // (the first Jacobian keeps all nine planes there: it may not fit where the later ones do); the second one
        // takes one cell per thread, so patches of at most 256 cells: 192 threads where every patch has at most 192
        // cells (tensor-product meshes: 160; compact patches of an unstructured mesh: 170-190), else 256.  Anything
        // else goes to the generic kernel, which loops over the cells.
        if (max_variant >= 3 && lean3_applies(c) && lean3_fits(c, jacobian, cmask)) return {3, 192, cmask};
        if (cells <= 256) return {2, cells <= 192 ? 192 : 256, cmask};
    }
    return {1, cells <= 192 ? 192 : 320, 0u};
}

AssemblyPath assembly_path(const Ctx &c, bool jacobian, int mode) { return assembly_path_upto(c, jacobian, mode, 3); }

// The generic patch kernel at T threads a workgroup, Jacobian or residual-only: every slice
template <int NS, bool PO, int NR, int CACHE, int T, bool LIN, bool TAB>
static void launch_patch(Ctx &c, bool jacobian, const StepCoef &sc, int mode) {
    constexpr int NEQ = NS + (PO ? 1 : 0);
    const int acc_doubles = jacobian ? c.pat.max_patch_width * NEQ * NEQ * SLICE : 0;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(c.pat.n_slices), dim3(T), patch_lds_bytes(c, jacobian), c.stream, c.d_model,
                           c.nv, c.d_slice_boff, c.d_patch_cell_ptr, c.d_patch_cells, c.d_patch_halo_ptr, c.d_patch_halo,
                           c.d_coords, c.d_u, c.d_uold, c.d_uold1, sc, c.d_ext[0], c.d_ext[1], c.d_ext[2], c.d_ext[3],
                           c.d_val, c.d_F, mode, acc_doubles, c.pat.max_patch_verts);
    };
    if (jacobian) launch(assemble_patch_kernel<NS, PO, NR, CACHE, T, LIN, TAB>);
    else launch(residual_patch_kernel<NS, PO, NR, CACHE, T, LIN, TAB>);
    note_assembly_launch(c, jacobian, 1, T, c.pat.n_slices);
}

// The row-phase kernel at T threads a workgroup: the n patches of `list` (null: the first n slices)
template <int NS, int NR, int T, bool TAB>
static void launch_lean2(Ctx &c, bool jacobian, const StepCoef &sc, int mode, uint32_t cmask, const int *list, int n) {
    if (n <= 0) return;
    const int acc_row = jacobian ? c.pat.max_patch_width * (NS + 1) * SLICE : 0;
    const size_t lds_bytes = lean2_lds_bytes(c, jacobian, LeanStash<NR>::N, T);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(n), dim3(T), lds_bytes, c.stream, c.d_model, c.nv, c.d_slice_boff,
                           c.d_patch_cell_ptr, c.d_patch_cells, c.d_patch_halo_ptr, c.d_patch_halo, c.d_coords, c.d_u,
                           c.d_uold, c.d_uold1, sc, c.d_ext[0], c.d_ext[1], c.d_ext[2], c.d_ext[3], c.d_val, c.d_F, mode,
                           acc_row, c.pat.max_patch_verts, c.xcd_remap ? 1 : 0, list, cmask);
    };
    if (jacobian) launch(assemble_lean2_kernel<NS, NR, T, TAB>);
    else launch(residual_lean2_kernel<NS, NR, T, TAB>);
    note_assembly_launch(c, jacobian, 2, T, n);
}

template <int NS, bool PO, int NR, int CACHE, bool LIN, bool TAB>
static void assemble_patch_t(Ctx &c, bool jacobian, int mode) {
    const StepCoef sc = step_coef(c.dt, c.dt_old);
    const AssemblyPath path = assembly_path(c, jacobian, mode);
    // The single case where "launched" may differ from "predicted": a third-generation launch that fails although it
    // was chosen (its plan not uploaded).  The assembly then takes what the decision gives without that generation:
    // the second one only where that takes every cell; otherwise the generic kernel assembles the whole mesh.
    const AssemblyPath fallback = path.variant == 3 ? assembly_path_upto(c, jacobian, mode, 2) : path;
    // (the condition is the model predicate's, at compile time: it only keeps the lean kernels from being instantiated
    // for models they do not exist for)
    if constexpr (PO && CACHE == 2 && NS >= 1 && !LIN) {
        if (path.variant >= 2) {
            // The patches of `list` (null: all n slices): the third generation (assemble3.hip) where it was chosen and
            // its launch succeeds, else the second (FEDM_ASSEMBLY_LEAN=2 keeps it) where that takes every cell; false: neither
            auto lean_launch = [&](const int *list, int n) {
                if (path.variant == 3 && launch_assemble_lean3(c, jacobian, list, n, path.cmask)) return true;
                if (fallback.variant != 2) return false;
                if (fallback.threads == 192) launch_lean2<NS, NR, 192, TAB>(c, jacobian, sc, mode, path.cmask, list, n);
                else launch_lean2<NS, NR, 256, TAB>(c, jacobian, sc, mode, path.cmask, list, n);
                return true;
            };
            bool done;
            if (c.halo_pending && c.comm && c.comm->d_patch_interior) {
                // the ghost values of the new state travel on the communication stream while the patches that stage no
                // ghost vertex are assembled ("ghost exchange overlapped with interior assembly"); the others follow it
                Comm &cm = *c.comm;
                comm_halo_begin(c);
                done = lean_launch(cm.d_patch_interior, cm.n_patch_interior);
                comm_halo_exchange(c, c.d_u);
                if (done) done = lean_launch(cm.d_patch_boundary, cm.n_patch_boundary);
                c.halo_pending = false;
            } else {
                flush_pending_halo(c);
                done = lean_launch(nullptr, c.pat.n_slices);
            }
            if (done) {
                if (jacobian) c.const_planes_valid = true;
                return;
            }
        }
    }
    // the generic kernel, for the whole mesh (variant 1: the decision's threads, or what is left of it)
    flush_pending_halo(c);
    if (fallback.threads == 192) launch_patch<NS, PO, NR, CACHE, 192, LIN, TAB>(c, jacobian, sc, mode);
    else launch_patch<NS, PO, NR, CACHE, 320, LIN, TAB>(c, jacobian, sc, mode);
    // every plane written, the constant ones included (the lean kernels may keep them from here on)
    if (jacobian && mode == 0) c.const_planes_valid = true;
}

template <int NS, bool PO, int NR, int CACHE, bool LIN, bool TAB>
static void assemble_variant_tab(Ctx &c, bool jacobian, int mode) {
    if (c.assembly_kind == 1) assemble_patch_t<NS, PO, NR, CACHE, LIN, TAB>(c, jacobian, mode);
    else assemble_colour_t<NS, PO, NR, CACHE, LIN, TAB>(c, jacobian, mode);
}

// a model with tabulated coefficient factors (Ctx::model_tables; it has a Poisson row: there is no |E| without one)
// takes the instantiations that look them up, every other model the ones without the look-up
template <int NS, bool PO, int NR, int CACHE, bool LIN = false>
static void assemble_variant(Ctx &c, bool jacobian, int mode) {
    if constexpr (PO) {
        if (c.model_tables) {
            assemble_variant_tab<NS, PO, NR, CACHE, LIN, true>(c, jacobian, mode);
            return;
        }
    }
    assemble_variant_tab<NS, PO, NR, CACHE, LIN, false>(c, jacobian, mode);
}

template <int NS, bool PO>
static void assemble_dispatch(Ctx &c, bool jacobian, int mode) {
    constexpr int NEQ = NS + (PO ? 1 : 0);
    const bool few = c.model.n_reactions <= 1;
    // cache exp(u) at the quadrature points when the tensors are emitted in several row passes
    const bool cache = NEQ > 1 && c.model.n_qp <= 3;
    const fedm_model_desc &m = c.model;
    const bool stdq = cache && fiat_degree2_rule(m);
    // the non-logarithmic representation runs on the generic (uncached, any reaction count) element only
    if (m.linear_representation) assemble_variant<NS, PO, FEDM_MAX_REACTIONS, 0, true>(c, jacobian, mode);
    else if (few && stdq) assemble_variant<NS, PO, 1, (NEQ > 1) ? 2 : 0>(c, jacobian, mode);
    // (the row-phase kernels take any number of reactions: element_lean.hpp stashes the rate coefficients of one
    // reaction beside the cell constants and evaluates several in each species row)
    else if (stdq) assemble_variant<NS, PO, FEDM_MAX_REACTIONS, (NEQ > 1) ? 2 : 0>(c, jacobian, mode);
    else if (few && cache) assemble_variant<NS, PO, 1, (NEQ > 1) ? 1 : 0>(c, jacobian, mode);
    else if (few) assemble_variant<NS, PO, 1, 0>(c, jacobian, mode);
    else if (cache) assemble_variant<NS, PO, FEDM_MAX_REACTIONS, (NEQ > 1) ? 1 : 0>(c, jacobian, mode);
    else assemble_variant<NS, PO, FEDM_MAX_REACTIONS, 0>(c, jacobian, mode);
}

void launch_assemble(Ctx &c, bool jacobian, int mode) {
    int *rec = c.launched[jacobian ? 1 : 0];   // what this assembly launches (note_assembly_launch)
    rec[0] = -1;
    rec[1] = rec[2] = rec[3] = 0;
    if (c.model_kind == 1) {
        flush_pending_halo(c);
        prof_begin(c, jacobian ? 0 : 2);
        launch_assemble_gd(c, jacobian, mode);
        prof_end(c);
        return;
    }
    if (jacobian) c.planes_fused = false;   // (set by the one-pass kernel when it forms the field split's planes itself)
    prof_begin(c, jacobian ? 0 : 2);  // the volume kernel only (all colours in variant 0)
    if (c.ns == 1 && !c.poisson) assemble_dispatch<1, false>(c, jacobian, mode);
    else if (c.ns == 1 && c.poisson) assemble_dispatch<1, true>(c, jacobian, mode);
    else if (c.ns == 2 && c.poisson) assemble_dispatch<2, true>(c, jacobian, mode);
    else if (c.ns == 2 && !c.poisson) assemble_dispatch<2, false>(c, jacobian, mode);
    else if (c.ns == 3 && c.poisson) assemble_dispatch<3, true>(c, jacobian, mode);
    else if (c.ns == 4 && c.poisson) assemble_dispatch<4, true>(c, jacobian, mode);
    prof_end(c);
    // dielectric layers: the Robin term and the charge's history in the Poisson rows, in both modes (the mirrored
    // facet terms come with the facets below, in the full assembly alone)
    if (c.diel) launch_layer_rows(c, jacobian, mode);
    if (mode == 0) {
        static const bool fuse_off = [] {
            const char *e = std::getenv("FEDM_FUSED_BOUNDARY");
            return e && e[0] == '0';
        }();
        // one GPU, patch assembly (the facets in one launch, with atomics), no row shared with a Dirichlet dof: the
        // facets go into launch_finalize's launch
        if (!fuse_off && !c.comm && c.n_owned == c.nv && !c.d_identity && c.assembly_kind == 1 && c.poisson &&
            c.n_bfacets > 0 && c.boundary_rows_disjoint && c.ns >= 1 && c.ns <= 4)
            c.boundary_pending = jacobian ? 2 : 1;
        else
            launch_boundary(c, jacobian);
    }
}

// The species equations alone (fedm_newton_solve_species): the species-only one-pass kernel where it applies, with the
// boundary facets' species columns behind it; otherwise the full assembly as it is (the solve ignores the potential
// row and column).  launch_finalize follows in both cases (Dirichlet and padding rows), then F of the potential rows
// is set to 0.
bool launch_assemble_species(Ctx &c, bool jacobian, bool volume_only) {
    bool one_pass = false;
    if (c.assembly_kind == 1 && c.ns == 2 && lean_model_applies(c)) {
        int *rec = c.launched[jacobian ? 1 : 0];
        const int saved[4] = {rec[0], rec[1], rec[2], rec[3]};
        rec[0] = -1;
        rec[1] = rec[2] = rec[3] = 0;
        prof_begin(c, jacobian ? 0 : 2);
        one_pass = launch_assemble_lean3_species(c, jacobian);
        prof_end(c);
        if (!one_pass)
            for (int i = 0; i < 4; ++i) rec[i] = saved[i];
    }
    if (jacobian && one_pass) c.planes_fused = false;
    if (one_pass && volume_only) return true;
    if (one_pass) {
        c.boundary_pending = 0;
        launch_boundary_species_cols(c, jacobian);
    } else {
        launch_assemble(c, jacobian, 0);
        if (volume_only) return false;
    }
    launch_finalize(c, jacobian, 0);
    launch_pick_entries(c, 0, 1.0, c.d_F, c.d_F);   // (in place: the kernel's pointers are not restrict-qualified)
    return one_pass;
}

}  // namespace fedm
