// Electrode currents (include/fedm_hip.h, fedm_currents_setup / fedm_currents_solve / fedm_currents): what the kernels
// and the C ABI in currents.hip share with the context's teardown.
#pragma once
#include "postproc.hpp"
#include "scalar_cg.hpp"

namespace fedm {

constexpr int CUR_MAX = FEDM_CURRENTS_MAX;
// slots of the cell pass's sums: a row of CUR_MAX per quantity
constexpr int CUR_COND = 0, CUR_DISP = CUR_MAX, CUR_COUP = 2 * CUR_MAX, CUR_CHARGE = 3 * CUR_MAX;
constexpr int CUR_SUMS = 4 * CUR_MAX;

// what the one-workgroup finish leaves for the one read-back
struct CurResult {
    double sum[CUR_SUMS];
    int not_finite, pad_;
};

struct Currents {
    int n_psi = 0;
    double *psi = nullptr;        // [CUR_MAX][nvp] the installed weighting potentials (padding stays 0)
    double cap[CUR_MAX][CUR_MAX] = {};   // the capacitance matrix of the installed potentials
    // slot-major partials of the cell pass, one entry per workgroup (postproc.hpp, POST_BLOCKS at the most)
    double *sum_part = nullptr;   // [CUR_SUMS][POST_BLOCKS]
    int *flag_part = nullptr;     // [POST_BLOCKS]
    CurResult *result = nullptr;
    // fedm_currents_solve (allocated at its first call): the candidates, one system and scalar_pcg's scratch
    double *psi_new = nullptr;    // [CUR_MAX][nvp]
    double *rhs = nullptr;        // [CUR_MAX][nvp] the caller's right-hand sides
    double *x = nullptr, *b = nullptr;   // [nvp] the free vertices' values and their right-hand side (0 on the unit rows)
    unsigned char *fixed = nullptr;      // [nvp] 1: a unit row of the operator (a conductor's vertex), and the padding
    ScalarCgWork cg;
};

#ifdef __HIPCC__
// ---- device: what the cell passes of currents.hip and circuit.hip share ------------------------------
// sum W grad a . grad b of two P1 functions on a cell: displacement and coupling with grad psi, the capacitance
__device__ __forceinline__ double cur_grad_dot(double cW, const double a[2], const double b[2]) {
    return cW * (a[0] * b[0] + a[1] * b[1]);
}

__device__ __forceinline__ void cur_grad(const double G[3][2], double p0, double p1, double p2, double g[2]) {
    g[0] = p0 * G[0][0] + p1 * G[1][0] + p2 * G[2][0];
    g[1] = p0 * G[0][1] + p1 * G[1][1] + p2 * G[2][1];
}

template <int K>
__device__ __forceinline__ void cur_write_partials(const double (&acc)[K], bool bad, double *__restrict__ sum_part,
                                                   int *__restrict__ flag_part) {
    __shared__ double lds_sum[K][POST_WAVES];
    const double s = block_sums(acc, lds_sum);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((int)threadIdx.x < K) sum_part[(size_t)threadIdx.x * POST_BLOCKS + blockIdx.x] = s;
    if (threadIdx.x == 0) flag_part[blockIdx.x] = any_bad;
}
#endif  // __HIPCC__

}  // namespace fedm
