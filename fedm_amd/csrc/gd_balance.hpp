// Particle and energy balance of LMEA models (include/fedm_hip.h, fedm_gd_balance): what the kernels and the C ABI in
// gd_balance.hip share with the context's teardown, and the value-only evaluation of the residual's point functions
// (unknowns, dme, semi-implicit mu, D, k, the drift-diffusion flux) in plain doubles -- gd.hip's gd_point,
// gd_rate_coefficient and gd_flux without the dual parts, operation by operation in their order.
#pragma once
#include "fedm_internal.hpp"

namespace fedm {

constexpr int BAL_GS = FEDM_GD_MAX_SPECIES, BAL_GR = FEDM_GD_MAX_REACTIONS;
// slots of the cell pass's sums
constexpr int BAL_CONTENT = 0, BAL_RATE = BAL_GS, BAL_REACTION = 2 * BAL_GS, BAL_LOSS = BAL_REACTION + BAL_GR,
              BAL_JOULE = BAL_LOSS + 1, BAL_CURRENT = BAL_JOULE + 1, BAL_GROUP0 = BAL_CURRENT + 1;
constexpr int BAL_CELL_SUMS = BAL_GROUP0 + FEDM_GD_BAL_MAX_GROUPS;
// slots of the facet pass's sums, per tag: wall[c], then the ion flux
constexpr int BAL_FACET_SUMS = BAL_GS + 1;
constexpr int BAL_NODAL = BAL_GS + 1;   // nodal maxima: the components below the potential, then u_0 - u_e

// what the one-workgroup finish leaves for the one read-back
struct BalResult {
    double sum[BAL_CELL_SUMS];
    double facet[BAL_FACET_SUMS][FEDM_MAX_TAGS];
    double field_max, centroid[2];
    double nodal_max[BAL_NODAL];
    int cell, vertex[BAL_NODAL];
    int not_finite, pad_;
};

// the facets of tag t + 1: entries [ptr[t], ptr[t + 1]) of the list, each cell * 3 + corner, in ascending order
struct BalFacets {
    int ptr[FEDM_MAX_TAGS + 1];
};

struct GdBalance {
    double *psi = nullptr;        // [nvp] weighting potential, or null
    int8_t *group = nullptr;      // [nvp] 0 or 1..n_groups, or null
    int n_groups = 0;
    BalFacets facets{};
    int *facet_list = nullptr;    // [facets.ptr[FEDM_MAX_TAGS]]
    // slot-major partials, one entry per workgroup (postproc.hpp, POST_BLOCKS at the most)
    double *sum_part = nullptr;   // [BAL_CELL_SUMS][POST_BLOCKS]
    double *facet_part = nullptr; // [BAL_FACET_SUMS][FEDM_MAX_TAGS]: a workgroup owns a tag
    double *max_part = nullptr;   // [1 + BAL_NODAL][POST_BLOCKS]: the field maximum, then the nodal maxima
    int *idx_part = nullptr;      // the same shape: where each maximum sits
    int *flag_part = nullptr;     // [2][POST_BLOCKS] + [FEDM_MAX_TAGS] not-finite flags of the cell, the vertex and the facet pass
    BalResult *result = nullptr;
};

#ifdef __HIPCC__
// ---- the residual's point functions, values only --------------------------------------------------
struct BalSG {   // value and spatial gradient of a scalar field at a point
    double v, gx, gy;
};

struct BalCell {
    double G[3][2], detJ, rn[3], x[3][2];
    int v[3];
};

__device__ __forceinline__ void bal_cell_init(BalCell &c, bool axisymmetric) {
    for (int a = 0; a < 3; ++a) c.rn[a] = axisymmetric ? c.x[a][0] : 0.5 / 3.14159265358979323846;
    const double d1x = c.x[1][0] - c.x[0][0], d1y = c.x[1][1] - c.x[0][1];
    const double d2x = c.x[2][0] - c.x[0][0], d2y = c.x[2][1] - c.x[0][1];
    const double det = d1x * d2y - d1y * d2x;
    c.detJ = fabs(det);
    c.G[0][0] = (c.x[1][1] - c.x[2][1]) / det;
    c.G[0][1] = (c.x[2][0] - c.x[1][0]) / det;
    c.G[1][0] = (c.x[2][1] - c.x[0][1]) / det;
    c.G[1][1] = (c.x[0][0] - c.x[2][0]) / det;
    c.G[2][0] = (c.x[0][1] - c.x[1][1]) / det;
    c.G[2][1] = (c.x[1][0] - c.x[0][0]) / det;
}

// the cell's vertices, coordinates and unknowns, then bal_cell_init; true: an unknown is not finite
template <int NEQ>
__device__ __forceinline__ bool bal_load_cell(int cell, const fedm_gd_desc *__restrict__ md,
                                              const double *__restrict__ coords, const int *__restrict__ cells,
                                              const double *__restrict__ u, BalCell &c, double U[3][NEQ]) {
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c.v[a] = cells[3 * (size_t)cell + a];
        c.x[a][0] = coords[2 * (size_t)c.v[a]];
        c.x[a][1] = coords[2 * (size_t)c.v[a] + 1];
#pragma unroll
        for (int e = 0; e < NEQ; ++e) {
            U[a][e] = u[(size_t)c.v[a] * NEQ + e];
            bad |= !isfinite(U[a][e]);
        }
    }
    bal_cell_init(c, md->axisymmetric != 0);
    return bad;
}

__device__ __forceinline__ BalSG bal_sg(double a0, double a1, double a2, const BalCell &c, const double phi[3]) {
    return {a0 * phi[0] + a1 * phi[1] + a2 * phi[2], a0 * c.G[0][0] + a1 * c.G[1][0] + a2 * c.G[2][0],
            a0 * c.G[0][1] + a1 * c.G[1][1] + a2 * c.G[2][1]};
}
// nodal field fi of the field table at the point
__device__ __forceinline__ BalSG bal_nodal(const double *__restrict__ fields, int nv, int fi, const BalCell &c,
                                           const double phi[3]) {
    const double *f = fields + (size_t)fi * nv;
    return bal_sg(f[c.v[0]], f[c.v[1]], f[c.v[2]], c, phi);
}
__device__ __forceinline__ double bal_nodal_value(const double *__restrict__ fields, int nv, int fi, const BalCell &c,
                                                  const double phi[3]) {
    const double *f = fields + (size_t)fi * nv;
    return f[c.v[0]] * phi[0] + f[c.v[1]] * phi[1] + f[c.v[2]] * phi[2];
}

template <int NEQ>
struct BalPoint {
    BalSG u[NEQ];          // unknowns: 0 energy, 1..ns-1 species, ns potential
    double e[NEQ - 1];     // exp(u_c), c < ns (e[0]: the energy density; the densities n_i for i >= 1)
    BalSG dme;             // change of the mean energy, fedm-gd.py:215
    double mu[NEQ - 1];    // semi-implicit mobilities (their value is all a flux takes)
    BalSG D[NEQ - 1];      // semi-implicit diffusion coefficients
    double Ex, Ey, me;     // E = -grad Phi; the current mean-energy Function (thermal velocity of electrons)
};

template <int NEQ>
__device__ __forceinline__ void bal_point(const double *__restrict__ fields, int nv, int nr, const BalCell &c,
                                          const double U[3][NEQ], const double phi[3], BalPoint<NEQ> &p) {
    constexpr int ns = NEQ - 1;
#pragma unroll
    for (int i = 0; i < NEQ; ++i) p.u[i] = bal_sg(U[0][i], U[1][i], U[2][i], c, phi);
    const int F_MU = 0, F_D = ns, F_MUD = 2 * ns, F_DD = 3 * ns, F_MEO = 4 * ns + 2 * nr, F_ME = F_MEO + 1,
              F_UEO = F_MEO + 2;
    const BalSG meo = bal_nodal(fields, nv, F_MEO, c, phi), ueo = bal_nodal(fields, nv, F_UEO, c, phi);
    p.me = bal_nodal_value(fields, nv, F_ME, c, phi);
    p.Ex = -p.u[NEQ - 1].gx;
    p.Ey = -p.u[NEQ - 1].gy;
#pragma unroll
    for (int i = 0; i < ns; ++i) p.e[i] = exp(p.u[i].v);
    {   // (sexp(u_0) - sexp(u_e) * meo) / sexp(ueo)
        const double e0 = p.e[0], ee = p.e[ns - 1], eo = exp(ueo.v);
        const BalSG E0 = {e0, e0 * p.u[0].gx, e0 * p.u[0].gy}, Ee = {ee, ee * p.u[ns - 1].gx, ee * p.u[ns - 1].gy};
        const BalSG num = {E0.v - Ee.v * meo.v, E0.gx - (Ee.gx * meo.v + Ee.v * meo.gx),
                           E0.gy - (Ee.gy * meo.v + Ee.v * meo.gy)};
        const BalSG Eo = {eo, eo * ueo.gx, eo * ueo.gy};
        const double inv = 1.0 / Eo.v;
        p.dme = {num.v * inv, (num.gx - num.v * inv * Eo.gx) * inv, (num.gy - num.v * inv * Eo.gy) * inv};
    }
#pragma unroll
    for (int i = 0; i < ns; ++i) {
        p.mu[i] = bal_nodal_value(fields, nv, F_MU + i, c, phi) + bal_nodal_value(fields, nv, F_MUD + i, c, phi) * p.dme.v;
        const BalSG Da = bal_nodal(fields, nv, F_D + i, c, phi), Db = bal_nodal(fields, nv, F_DD + i, c, phi);
        p.D[i] = {Da.v + Db.v * p.dme.v, Da.gx + (Db.gx * p.dme.v + Db.v * p.dme.gx),
                  Da.gy + (Db.gy * p.dme.v + Db.v * p.dme.gy)};
    }
}

// semi-implicit rate coefficient of reaction j at the point
__device__ __forceinline__ double bal_rate_coefficient(const double *__restrict__ fields, int nv, int ns, int nr, int j,
                                                       const BalCell &c, const double phi[3], double dme) {
    return bal_nodal_value(fields, nv, 4 * ns + j, c, phi) + bal_nodal_value(fields, nv, 4 * ns + nr + j, c, phi) * dme;
}

// drift-diffusion flux, fedm/functions.py:219-237; e = exp(ulog.v)
__device__ __forceinline__ void bal_flux(double sign, const BalSG &ulog, double e, const BalSG &D, double mu, double Ex,
                                         double Ey, bool grad_diffusion, double &gx, double &gy) {
    const double egx = e * ulog.gx, egy = e * ulog.gy;
    if (grad_diffusion) {
        gx = -(D.gx * e + D.v * egx);
        gy = -(D.gy * e + D.v * egy);
    } else {
        gx = -(D.v * egx);
        gy = -(D.v * egy);
    }
    gx = gx + sign * (mu * Ex * e);
    gy = gy + sign * (mu * Ey * e);
}

// the flux of species s >= 1 as its row of the residual has it: 0 for 'reaction', -grad(D exp(u)) for
// 'diffusion-reaction' (functions.py:362-364), the drift-diffusion flux otherwise
template <int NEQ>
__device__ __forceinline__ void bal_species_flux(const fedm_gd_desc *__restrict__ md, const BalPoint<NEQ> &p, int s,
                                                 double &gx, double &gy) {
    const int et = md->eq_type[s];
    gx = gy = 0.0;
    if (et == FEDM_EQ_DRIFT_DIFFUSION_REACTION)
        bal_flux(md->sign[s], p.u[s], p.e[s], p.D[s], p.mu[s], p.Ex, p.Ey, md->grad_diffusion[s] != 0, gx, gy);
    else if (et == FEDM_EQ_DIFFUSION_REACTION)
        bal_flux(0.0, p.u[s], p.e[s], p.D[s], 0.0, 0.0, 0.0, true, gx, gy);
}
#endif  // __HIPCC__

}  // namespace fedm
