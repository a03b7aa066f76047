// What the post-processing passes over the resident state share -- photoionisation (photo.hip, photo_abi.cpp),
// diagnostics (diag.hip), field output (fields.hip, gd_fields.hip), the LMEA balance (gd_balance.hip) and the electrode
// currents (currents.hip) -- and nobody else includes.  Their pattern: a first pass writes slot-major partials in a fixed
// order, one workgroup finishes them, one read-back, and every bad argument is refused with a message.  Host side: the
// refusal, device arrays, the vertices' cell lists, the upload of a scalar solve's hierarchy (the solver itself is
// scalar_cg.hpp's), the read-back, the two families' dispatch and the weighting potential's set-up.  Device side: the
// reductions' cores, one copy each, so that a change of the order or of the tie rule reaches every pass that promises
// bitwise reproducibility with it.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>

#include "solver.hpp"
#ifdef __HIPCC__
#include <climits>

#include "device_util.hpp"
#endif

namespace fedm {

// ---- host ------------------------------------------------------------------------------------------
// sets the error to "who: why", returns -2
inline int refuse(const char *who, const std::string &why) {
    set_error(std::string(who) + ": " + why);
    return -2;
}

// n entries on the device (one at the least), copied from src or, src null, zero
template <class T>
int device_array(T *&dst, const T *src, size_t n) {
    FEDM_HIP_CHECK(hipMalloc((void **)&dst, sizeof(T) * std::max<size_t>(n, 1)));
    if (src) FEDM_HIP_CHECK(hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
    else FEDM_HIP_CHECK(hipMemset(dst, 0, sizeof(T) * std::max<size_t>(n, 1)));
    return 0;
}

// vertex -> its (cell, corner) pairs: v_ptr[nv + 1], and v_idx[3 nc] = cell * 3 + corner, ascending within a vertex --
// the order of every sum over a vertex's cells
inline void vertex_cell_lists(int nv, const std::vector<int> &cells, std::vector<int> &v_ptr, std::vector<int> &v_idx) {
    v_ptr.assign((size_t)nv + 1, 0);
    v_idx.resize(cells.size());
    for (size_t k = 0; k < cells.size(); ++k) ++v_ptr[cells[k] + 1];
    for (int v = 0; v < nv; ++v) v_ptr[v + 1] += v_ptr[v];
    std::vector<int> fill(v_ptr.begin(), v_ptr.end() - 1);
    for (size_t k = 0; k < cells.size(); ++k) v_idx[fill[cells[k]]++] = (int)k;
}

// What scalar_pcg solves with, from one fedm_photo_hierarchy of c.nv vertices: the finest operator in double precision
// into A and, with more than one level, its V-cycles (plain sweeps on every level: composite operators from level
// n_levels + 1 on, i.e. nowhere) into M, which stays null for Jacobi.  `what` goes before the reason of a refusal
// ("term 2: " or nothing).  On an error (-1, -2) the caller releases what has been made, with release_hierarchy.
inline int upload_hierarchy(Ctx &c, const char *who, const std::string &what, const fedm_photo_hierarchy &t, EllMat &A,
                            Amg *&M) {
    if (t.n_levels < 1 || !t.A || (t.n_levels > 1 && (!t.P || !t.R || !t.coarse_inverse || t.nu < 1)))
        return refuse(who, what + "bad hierarchy (levels with their prolongators, restrictions and a dense coarsest inverse; "
                                  "V(nu,nu) with nu >= 1)");
    const fedm_csr &A0 = t.A[0];
    if (A0.n_rows != c.nv || A0.n_cols != c.nv || !A0.indptr || !A0.indices || !A0.values)
        return refuse(who, what + "the operator has " + std::to_string(A0.n_rows) + " rows, the mesh " +
                               std::to_string(c.nv) + " vertices");
    A.single = false;
    if (const int rc = A.from_csr(A0, true)) {
        set_error(std::string(who) + ": " + what + "operator upload failed (bad CSR or out of memory)");
        return rc < -1 ? -2 : -1;
    }
    if (A.n_rows_p != c.nvp) return refuse(who, what + "the operator's padded rows differ from the context's");
    if (t.n_levels == 1) return 0;
    return build_amg(c, c.nv, t.n_levels, t.A, t.P, t.R, t.coarse_inverse, t.nu, t.omega, &M, t.n_levels + 1);
}
inline void release_hierarchy(EllMat &A, Amg *&M) {
    A.release();
    if (M) M->release();
    delete M;
    M = nullptr;
}

// the one read-back of a call: what the finish left, once the stream has run dry, and any launch's error
template <class T>
int read_result(Ctx &c, T &host, const T *dev) {
    FEDM_HIP_CHECK(hipMemcpyAsync(&host, dev, sizeof(T), hipMemcpyDeviceToHost, c.stream));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// The LFA model's compile-time switches from its run-time flags: fn(NS, PO, TAB) -- the instantiations the assembly has
// (one or two species without a Poisson equation, one to four with; tables need |E|, hence a Poisson equation)
template <class Fn>
void with_model_flags(const Ctx &c, Fn &&fn) {
    auto tab = [&](auto ns) {
        if (c.model_tables) fn(ns, std::true_type{}, std::true_type{});
        else fn(ns, std::true_type{}, std::false_type{});
    };
    if (!c.poisson) {
        if (c.ns == 1) fn(std::integral_constant<int, 1>{}, std::false_type{}, std::false_type{});
        else fn(std::integral_constant<int, 2>{}, std::false_type{}, std::false_type{});
        return;
    }
    switch (c.ns) {
        case 1: tab(std::integral_constant<int, 1>{}); break;
        case 2: tab(std::integral_constant<int, 2>{}); break;
        case 3: tab(std::integral_constant<int, 3>{}); break;
        default: tab(std::integral_constant<int, 4>{}); break;
    }
}

// The LMEA model's equation count as a compile-time number: fn(NEQ), 3 to 6, what launch_assemble_gd instantiates.  The
// caller has refused every other count, with its own message.
template <class Fn>
void with_gd_neq(const Ctx &c, Fn &&fn) {
    switch (c.neq) {
        case 3: fn(std::integral_constant<int, 3>{}); break;
        case 4: fn(std::integral_constant<int, 4>{}); break;
        case 5: fn(std::integral_constant<int, 5>{}); break;
        default: fn(std::integral_constant<int, 6>{}); break;
    }
}

// A weighting potential and vertex groups 1..n_groups for a pass (fedm_diag_setup, fedm_gd_balance_setup): the refusals,
// then `ensure(c)` makes the pass's buffers at need (0, or its error), then psi, group and n_groups of *holder are
// replaced by nvp-padded, zero-filled copies (null: none).  The stream runs dry before the old arrays go.
template <class Pass, class Ensure>
int weighting_setup(Ctx &c, const char *who, int max_groups, bool groups_need_poisson, const double *psi,
                    const int8_t *group, int n_groups, Pass *&holder, Ensure &&ensure) {
    if (n_groups < 0 || n_groups > max_groups)
        return refuse(who, std::to_string(n_groups) + " groups, 0 to " + std::to_string(max_groups) + " are possible");
    if ((n_groups > 0) != (group != nullptr)) return refuse(who, "groups go with their array and the array with n_groups > 0");
    if (groups_need_poisson && group && !c.poisson)
        return refuse(who, "vertex groups need the Poisson row, and the model has no Poisson equation");
    for (int v = 0; group && v < c.nv; ++v)
        if (group[v] < 0 || group[v] > n_groups)
            return refuse(who, "group[" + std::to_string(v) + "] = " + std::to_string((int)group[v]) + " outside 0.." +
                                   std::to_string(n_groups));
    for (int v = 0; psi && v < c.nv; ++v)
        if (!std::isfinite(psi[v])) return refuse(who, "psi[" + std::to_string(v) + "] is not finite");
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (const int rc = ensure(c)) return rc;
    Pass &d = *holder;
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (d.psi) hipFree(d.psi);
    if (d.group) hipFree(d.group);
    d.psi = nullptr;
    d.group = nullptr;
    d.n_groups = 0;
    if (psi) {
        FEDM_HIP_CHECK(hipMalloc((void **)&d.psi, sizeof(double) * c.nvp));
        FEDM_HIP_CHECK(hipMemset(d.psi, 0, sizeof(double) * c.nvp));
        FEDM_HIP_CHECK(hipMemcpy(d.psi, psi, sizeof(double) * c.nv, hipMemcpyHostToDevice));
    }
    if (group) {
        FEDM_HIP_CHECK(hipMalloc((void **)&d.group, c.nvp));
        FEDM_HIP_CHECK(hipMemset(d.group, 0, c.nvp));
        FEDM_HIP_CHECK(hipMemcpy(d.group, group, c.nv, hipMemcpyHostToDevice));
        d.n_groups = n_groups;
    }
    return 0;
}

#ifdef __HIPCC__
// ---- device: the reductions ----------------------------------------------------------------------
// Workgroups of a reduction's first pass at the most (beyond: a stride loop), and their threads.  The finish is one
// workgroup with one thread per first-pass workgroup, so the two must be equal.
constexpr int POST_BLOCKS = 256;
constexpr int POST_THREADS = 256;
static_assert(POST_BLOCKS == POST_THREADS, "the finish kernels bring one first-pass workgroup's partials per thread");
constexpr int POST_WAVES = POST_THREADS / 64;

// a maximum with the index it sits at; on an exact tie the lower index stays.  Nothing compares greater than or equal
// to a NaN, so a NaN is never taken: the not-finite flag reports it.
struct MaxIdx {
    double v;
    int i;
    __device__ __forceinline__ void take(double ov, int oi) {
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
};

__device__ __forceinline__ MaxIdx wave_max(MaxIdx m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(m.v, off, 64);
        const int oi = __shfl_down(m.i, off, 64);
        m.take(ov, oi);
    }
    return m;
}

// K values per thread -> K sums in the threads 0 .. K - 1 (thread k holds sum k): lanes by shuffles, then the waves
// in ascending order
template <int K>
__device__ __forceinline__ double block_sums(const double (&v)[K], double (*lds)[POST_WAVES]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) lds[k][wave] = s;
    }
    __syncthreads();
    double s = 0.0;
    if ((int)threadIdx.x < K)
        for (int w = 0; w < POST_WAVES; ++w) s += lds[threadIdx.x][w];
    __syncthreads();
    return s;
}

// K maxima per thread -> thread k holds maximum k
template <int K>
__device__ __forceinline__ MaxIdx block_maxes(const MaxIdx (&m)[K], double (*lv)[POST_WAVES], int (*li)[POST_WAVES]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const MaxIdx r = wave_max(m[k]);
        if (lane == 0) {
            lv[k][wave] = r.v;
            li[k][wave] = r.i;
        }
    }
    __syncthreads();
    MaxIdx r{-INFINITY, INT_MAX};
    if ((int)threadIdx.x < K)
        for (int w = 0; w < POST_WAVES; ++w) r.take(lv[threadIdx.x][w], li[threadIdx.x][w]);
    __syncthreads();
    return r;
}

// the centroid of a cell, for the finish that found a maximum there
__device__ __forceinline__ void cell_centroid(const double *__restrict__ coords, const int *__restrict__ cells, int cell,
                                              double &r, double &z) {
    const int v0 = cells[3 * (size_t)cell], v1 = cells[3 * (size_t)cell + 1], v2 = cells[3 * (size_t)cell + 2];
    r = (coords[2 * (size_t)v0] + coords[2 * (size_t)v1] + coords[2 * (size_t)v2]) / 3.0;
    z = (coords[2 * (size_t)v0 + 1] + coords[2 * (size_t)v1 + 1] + coords[2 * (size_t)v2 + 1]) / 3.0;
}
#endif  // __HIPCC__

}  // namespace fedm
