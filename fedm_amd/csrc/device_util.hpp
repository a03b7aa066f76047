// Device helpers shared by assemble.hip, assemble3.hip, spmv.hip and kernels.hip -- only what more than one of them uses.
#pragma once
#include <hip/hip_runtime.h>

namespace fedm {

// Workgroups b, b + 8, b + 16, ... are observed to share an XCD (round-robin dispatch; a speed
// heuristic, never relied upon for correctness): give every XCD a contiguous range of patches so
// that the halo vertices two neighbouring patches both stage are served by ONE L2.
__device__ __forceinline__ int xcd_contiguous(int b, int n) {
    const int per = n >> 3, full = per << 3;
    return b < full ? (b & 7) * per + (b >> 3) : b;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

struct PtrPack8 {
    const double *p[8];
};

}  // namespace fedm
