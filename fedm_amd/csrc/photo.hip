// Photoionisation in the three-term Helmholtz approximation (include/fedm_hip.h, fedm_photo_setup): the load vector
// of the ionisation rate at u_old and the source tables the element routines read; the terms' solves between the two
// are scalar_cg.hip's.  Plain launches on the context's stream; no kernel waits for another workgroup and none adds with
// atomics: every sum has a fixed order, so an update is bitwise reproducible.
#include "photo.hpp"

#include <cmath>

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

}  // namespace fedm
