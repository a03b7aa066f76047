// Field output of LMEA models (include/fedm_hip.h, fedm_gd_fields_setup / fedm_gd_probe_setup / fedm_gd_fields): derived
// nodal fields and point probes from the resident state and the field table, where the residual of gd.hip evaluates them.
// One pass over the cells for ALL projected requests of the call (a thread per cell evaluates gd_balance.hpp's
// bal_point once per quadrature point and stores its three corner entries per request) and one over the vertices (a
// thread per (vertex, request): pointwise kinds from the state, the descriptor and the table, projected kinds by adding
// the vertex's entries in the ascending (cell, corner) order of the list).  The vertex lists, the lumped mass, the
// consistent solve, the blend, the probes and the read-back are fields.hip's (fields.hpp).  Plain launches on the
// context's stream; no kernel caps its grid, none waits for another workgroup, and nothing adds with floating-point
// atomics: a call is bitwise reproducible.  It reads the state and the table and writes neither.
#include <cmath>
#include <string>

#include "fields.hpp"
#include "gd_balance.hpp"
#include "postproc.hpp"
#include "solver.hpp"

namespace fedm {

// what a call's projected requests need of a point, decided on the host: the branches on it are wave-uniform
constexpr int GDF_NEED_POINT = 1, GDF_NEED_REACTIONS = 2, GDF_NEED_FLUXES = 4;

// the projected requests of a call: slot k of cell_b belongs to request req[k] of the call
struct GdFieldCellReqs {
    int n, need;
    int kind[FEDM_FIELDS_MAX_REQ], index[FEDM_FIELDS_MAX_REQ];
};
// every request of a call: slot[k] >= 0: its slot of cell_b (projected), -1: pointwise
struct GdFieldVertexReqs {
    int n;
    int kind[FEDM_FIELDS_MAX_REQ], index[FEDM_FIELDS_MAX_REQ], slot[FEDM_FIELDS_MAX_REQ];
};

// ---- the cells -------------------------------------------------------------------------------------
// A thread per cell.  Per quadrature point the integrands f_k of all requests, then acc[k][a] += W f_k phi_a with the
// plain measure W = qp_w |det J|.  The request loops are unrolled to FEDM_FIELDS_MAX_REQ with a guard, the species'
// loops to the model's count: integrands and accumulators are indexed by compile-time numbers only (registers, never
// scratch); a request's kind and index are kernel arguments, the same in every lane.  The reaction loop stays rolled
// (gd_balance.hip says what unrolling it cost).
template <int NEQ>
__global__ __launch_bounds__(FIELDS_THREADS) void gd_fields_cell_kernel(int nc, int nv, const fedm_gd_desc *__restrict__ md,
                                                                        const double *__restrict__ fields,
                                                                        const double *__restrict__ coords,
                                                                        const int *__restrict__ cells,
                                                                        const double *__restrict__ u, GdFieldCellReqs rq,
                                                                        double *__restrict__ cell_b) {
    constexpr int ns = NEQ - 1, IPHI = NEQ - 1, ie = ns - 1, K = FEDM_FIELDS_MAX_REQ;
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= nc) return;
    BalCell c;
    double U[3][NEQ];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c.v[a] = cells[3 * (size_t)cell + a];
        c.x[a][0] = coords[2 * (size_t)c.v[a]];
        c.x[a][1] = coords[2 * (size_t)c.v[a] + 1];
#pragma unroll
        for (int e = 0; e < NEQ; ++e) U[a][e] = u[(size_t)c.v[a] * NEQ + e];
    }
    bal_cell_init(c, md->axisymmetric != 0);
    double gP[2] = {0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        gP[0] += U[a][IPHI] * c.G[a][0];
        gP[1] += U[a][IPHI] * c.G[a][1];
    }
    const double Em = sqrt(gP[0] * gP[0] + gP[1] * gP[1]);
    const int nr = md->n_reactions, nq = md->n_qp;
    const bool need_point = (rq.need & GDF_NEED_POINT) != 0, need_reac = (rq.need & GDF_NEED_REACTIONS) != 0,
               need_flux = (rq.need & GDF_NEED_FLUXES) != 0;
    double acc[K][3];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
    for (int q = 0; q < nq; ++q) {
        const double phi[3] = {1.0 - md->qp_x[q] - md->qp_y[q], md->qp_x[q], md->qp_y[q]};
        const double W = md->qp_w[q] * c.detJ;
        double f[K];
        // the kinds of the potential alone: constant over the cell
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int kind = rq.kind[k];
            f[k] = 0.0;
            if (k >= rq.n) continue;
            if (kind == FEDM_GD_FIELD_E_R) f[k] = -gP[0];
            else if (kind == FEDM_GD_FIELD_E_Z) f[k] = -gP[1];
            else if (kind == FEDM_GD_FIELD_E_NORM) f[k] = Em;
            else if (kind == FEDM_GD_FIELD_REDUCED_FIELD) f[k] = 1e21 * Em / md->N0;
        }
        if (need_point) {
            BalPoint<NEQ> p;
            bal_point<NEQ>(fields, nv, nr, c, U, phi, p);
            if (need_reac) {
                // Source_term / Energy_Source_term (functions.py:835-843, 901-912), as gd.hip and gd_balance.hip take them
                double me_arg = 0.0;
                if (md->mean_energy_form == FEDM_GD_ME_UNKNOWN_RATIO) me_arg = p.u[0].v / p.u[ie].v;
#pragma unroll 1
                for (int j = 0; j < nr; ++j) {
                    double rate = bal_rate_coefficient(fields, nv, ns, nr, j, c, phi, p.dme.v);
#pragma unroll
                    for (int i = 0; i < ns; ++i)
                        for (int e = 0; e < md->power[j][i]; ++e) rate = (i == 0) ? rate * md->N0 : rate * p.e[i];
                    const double lj = md->energy_loss[j];   // functions.py:905-911
                    double lr;
                    if (lj > 7e77 && lj < 8e77) lr = (md->energy_Ei - me_arg) * rate;
                    else if (lj > 9e99 && lj < 1e100) lr = me_arg * rate;
                    else lr = lj * rate;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        if (k >= rq.n) continue;
                        const int kind = rq.kind[k], idx = rq.index[k];
                        if (kind == FEDM_GD_FIELD_RATE) {
                            if (idx == j) f[k] = rate;
                        } else if (kind == FEDM_GD_FIELD_SOURCE) {
                            f[k] = f[k] + (double)md->net[j][idx] * rate;
                        } else if (kind == FEDM_GD_FIELD_COLLISION_LOSS) {
                            f[k] += lr;
                        }
                    }
                }
            }
            if (need_flux) {
                // the species rows' fluxes; the electrons' is Joule heating's too (fedm-gd.py:359)
                double cur[2] = {0.0, 0.0};
#pragma unroll
                for (int s = 1; s < ns; ++s) {
                    double gx, gy;
                    bal_species_flux<NEQ>(md, p, s, gx, gy);
                    cur[0] += md->sign[s] * gx;
                    cur[1] += md->sign[s] * gy;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        if (k >= rq.n || rq.index[k] != s) continue;
                        if (rq.kind[k] == FEDM_GD_FIELD_FLUX_R) f[k] = gx;
                        else if (rq.kind[k] == FEDM_GD_FIELD_FLUX_Z) f[k] = gy;
                    }
                    if (s == ie) {
                        const double joule = -(gx * p.Ex + gy * p.Ey);
#pragma unroll
                        for (int k = 0; k < K; ++k)
                            if (k < rq.n && rq.kind[k] == FEDM_GD_FIELD_JOULE) f[k] = joule;
                    }
                }
                // the energy row's flux: 5/3 of the electrons' coefficients on the energy unknown (gd.hip, fedm-gd.py:354)
                double wx, wy;
                const BalSG D53 = {p.D[ie].v * (5.0 / 3.0), p.D[ie].gx * (5.0 / 3.0), p.D[ie].gy * (5.0 / 3.0)};
                bal_flux(md->sign[ie], p.u[0], p.e[0], D53, p.mu[ie] * (5.0 / 3.0), p.Ex, p.Ey, md->grad_diffusion[ie] != 0,
                         wx, wy);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (k >= rq.n) continue;
                    const int kind = rq.kind[k];
                    if (kind == FEDM_GD_FIELD_CURRENT_R) f[k] = FEDM_ELEMENTARY_CHARGE * cur[0];
                    else if (kind == FEDM_GD_FIELD_CURRENT_Z) f[k] = FEDM_ELEMENTARY_CHARGE * cur[1];
                    else if (kind == FEDM_GD_FIELD_FLUX_R && rq.index[k] == 0) f[k] = wx;
                    else if (kind == FEDM_GD_FIELD_FLUX_Z && rq.index[k] == 0) f[k] = wy;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double Wf = W * f[k];
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[k][a] += Wf * phi[a];
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k >= rq.n) continue;
        double *dst = cell_b + ((size_t)k * nc + cell) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) dst[a] = acc[k][a];
    }
}

// ---- the vertices ----------------------------------------------------------------------------------
// A thread per (vertex, request), blockIdx.y the request.  Pointwise kinds from the state, the descriptor and the table;
// projected kinds: the vertex's entries in the order of the list, divided by the lumped mass or (raw_sums) left as the
// right-hand side of the consistent solve.  The padding gets 0.  Request 0's threads look at every component of the
// state for the flag; every result is looked at as well (fields_vertex_kernel's rule).
__global__ __launch_bounds__(FIELDS_THREADS) void gd_fields_vertex_kernel(
    int nv, int nvp, int nc, int ns, const fedm_gd_desc *__restrict__ md, const double *__restrict__ fields,
    const double *__restrict__ u, const int *__restrict__ v_ptr, const int *__restrict__ v_idx, const double *__restrict__ m,
    const double *__restrict__ cell_b, GdFieldVertexReqs rq, int raw_sums, double *__restrict__ dst, int *__restrict__ flag) {
#pragma clang fp contract(off)
    const int v = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (v >= nvp) return;
    const int neq = ns + 1;
    double val = 0.0;
    bool bad = false;
    if (v < nv) {
        const int kind = rq.kind[k], idx = rq.index[k], slot = rq.slot[k];
        if (k == 0)
            for (int e = 0; e < neq; ++e) bad |= !isfinite(u[(size_t)v * neq + e]);
        if (slot >= 0) {
            const double *b = cell_b + (size_t)slot * nc * 3;
            double s = 0.0;
            for (int j = v_ptr[v]; j < v_ptr[v + 1]; ++j) s += b[v_idx[j]];
            val = raw_sums ? s : s / m[v];
        } else if (kind == FEDM_GD_FIELD_STATE) {
            val = u[(size_t)v * neq + idx];
        } else if (kind == FEDM_GD_FIELD_DENSITY) {
            val = exp(u[(size_t)v * neq + idx]);
        } else if (kind == FEDM_GD_FIELD_CHARGE) {
            double s = 0.0;
            for (int i = 1; i < ns; ++i) s += md->sign[i] * exp(u[(size_t)v * neq + i]);
            val = FEDM_ELEMENTARY_CHARGE * s;
        } else if (kind == FEDM_GD_FIELD_MEAN_ENERGY) {   // gdprep.hip's gd_mean_energy_kernel
            val = exp(u[(size_t)v * neq] - u[(size_t)v * neq + (neq - 2)]);
        } else {   // TABLE
            val = fields[(size_t)idx * nv + v];
        }
        bad |= !isfinite(val);
    }
    dst[(size_t)k * nvp + v] = val;
    if (bad) atomicOr(flag, 1);
}

namespace {

bool gd_projected(int kind) { return kind >= FEDM_GD_FIELD_E_R && kind <= FEDM_GD_FIELD_CURRENT_Z; }
// evaluated as the residual of the current step evaluates it: u_new and the table as it stands, no state selector
bool gd_of_the_step(int kind) { return kind == FEDM_GD_FIELD_TABLE || (kind >= FEDM_GD_FIELD_RATE && kind <= FEDM_GD_FIELD_CURRENT_Z); }

const char *gd_kind_name(int kind) {
    static const char *names[] = {"STATE", "DENSITY", "CHARGE", "MEAN_ENERGY", "TABLE", "E_R", "E_Z", "E_NORM", "REDUCED_FIELD",
                                  "RATE", "SOURCE", "COLLISION_LOSS", "JOULE", "FLUX_R", "FLUX_Z", "CURRENT_R", "CURRENT_Z"};
    return names[kind - FEDM_GD_FIELD_STATE];
}

int gd_check_ctx(const Ctx &c, const char *who) {
    if (c.model_kind != 1)
        return refuse(who, "an LFA context (these are the LMEA family's fields; fedm_fields has the LFA family's)");
    if (c.n_owned != c.nv) return refuse(who, "a context with ghost vertices (one GPU only)");
    if (c.neq < 3 || c.neq > 6) return refuse(who, std::to_string(c.neq) + " equations: 3 to 6 are built");
    return 0;
}

template <int NEQ>
void launch_gd_cells(Ctx &c, const double *u, const GdFieldCellReqs &cq) {
    hipLaunchKernelGGL((gd_fields_cell_kernel<NEQ>), dim3((c.nc + FIELDS_THREADS - 1) / FIELDS_THREADS), dim3(FIELDS_THREADS),
                       0, c.stream, c.nc, c.nv, c.d_gd, c.d_gd_fields, c.d_coords, c.d_cells, u, cq, c.fields->cell_b);
}

}  // namespace
}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_gd_fields_setup(fedm_ctx *h, const fedm_csr *mass) {
    const char *who = "fedm_gd_fields_setup";
    if (!h) return refuse(who, "null context");
    Ctx &c = h->c;
    if (const int rc = gd_check_ctx(c, who)) return rc;
    return fields_setup_shared(c, mass, who);
}

int fedm_gd_probe_setup(fedm_ctx *h, int n_points, const int32_t *vertices, const double *weights) {
    const char *who = "fedm_gd_probe_setup";
    if (!h) return refuse(who, "null context");
    Ctx &c = h->c;
    if (const int rc = gd_check_ctx(c, who)) return rc;
    return fields_probe_setup_shared(c, n_points, vertices, weights, who, "fedm_gd_fields_setup");
}

int fedm_gd_fields(fedm_ctx *h, const fedm_field_opts *opts, int n_req, const fedm_field_req *req, double *nodal,
                   double *probes, int32_t *finite, int32_t *cg_iterations) {
    const char *who = "fedm_gd_fields";
    if (!h || !opts || !req || !finite) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (const int rc = gd_check_ctx(c, who)) return rc;
    if (const int rc = fields_check_opts(c, *opts, n_req, who, "fedm_gd_fields_setup")) return rc;
    const int ns = c.gd.n_species, nr = c.gd.n_reactions;
    GdFieldCellReqs cq{};
    GdFieldVertexReqs vq{};
    vq.n = n_req;
    for (int k = 0; k < n_req; ++k) {
        const int kind = req[k].kind, idx = req[k].index;
        const std::string r = "request " + std::to_string(k) + ": ";
        int first = 0, limit = 1;   // indices first .. limit - 1
        switch (kind) {
            case FEDM_GD_FIELD_STATE: limit = c.neq; break;
            case FEDM_GD_FIELD_DENSITY:
            case FEDM_GD_FIELD_FLUX_R:
            case FEDM_GD_FIELD_FLUX_Z: limit = ns; break;
            case FEDM_GD_FIELD_SOURCE: first = 1; limit = ns; break;
            case FEDM_GD_FIELD_TABLE: limit = c.gd_n_fields; break;
            case FEDM_GD_FIELD_RATE: limit = nr; break;
            case FEDM_GD_FIELD_CHARGE:
            case FEDM_GD_FIELD_MEAN_ENERGY:
            case FEDM_GD_FIELD_E_R:
            case FEDM_GD_FIELD_E_Z:
            case FEDM_GD_FIELD_E_NORM:
            case FEDM_GD_FIELD_REDUCED_FIELD:
            case FEDM_GD_FIELD_COLLISION_LOSS:
            case FEDM_GD_FIELD_JOULE:
            case FEDM_GD_FIELD_CURRENT_R:
            case FEDM_GD_FIELD_CURRENT_Z: break;
            default: return refuse(who, r + "unknown kind " + std::to_string(kind));
        }
        if (idx < first || idx >= limit)
            return refuse(who, r + "index " + std::to_string(idx) + " out of range (" + std::to_string(first) + " to " +
                                   std::to_string(limit - 1) + ")");
        if (gd_of_the_step(kind) && opts->num != opts->den)
            return refuse(who, r + gd_kind_name(kind) + " is what the residual of the current step evaluates (u_new, the "
                                   "field table as it stands): no blend, num == den only");
        vq.kind[k] = kind;
        vq.index[k] = idx;
        vq.slot[k] = -1;
        if (gd_projected(kind)) {
            vq.slot[k] = cq.n;
            cq.kind[cq.n] = kind;
            cq.index[cq.n] = idx;
            ++cq.n;
            if (kind >= FEDM_GD_FIELD_RATE) cq.need |= GDF_NEED_POINT;
            if (kind == FEDM_GD_FIELD_RATE || kind == FEDM_GD_FIELD_SOURCE || kind == FEDM_GD_FIELD_COLLISION_LOSS)
                cq.need |= GDF_NEED_REACTIONS;
            if (kind >= FEDM_GD_FIELD_JOULE) cq.need |= GDF_NEED_FLUXES;
        }
    }
    if (const int rc = fields_check_projection(c, *opts, probes != nullptr, who, "fedm_gd_fields_setup", "fedm_gd_probe_setup"))
        return rc;
    Fields &f = *c.fields;
    return fields_run(c, *opts, n_req, vq.slot, cq.n > 0,
                      [&](const double *u, int raw_sums, double *dst) {
                          // (gd_check_ctx has refused the equation counts that are not built)
                          if (cq.n > 0) with_gd_neq(c, [&](auto neq) { launch_gd_cells<decltype(neq)::value>(c, u, cq); });
                          hipLaunchKernelGGL(gd_fields_vertex_kernel, dim3((c.nvp + FIELDS_THREADS - 1) / FIELDS_THREADS, vq.n),
                                             dim3(FIELDS_THREADS), 0, c.stream, c.nv, c.nvp, c.nc, ns, c.d_gd, c.d_gd_fields, u,
                                             f.v_ptr, f.v_idx, f.m, f.cell_b, vq, raw_sums, dst, f.flag);
                      },
                      nodal, probes, finite, cg_iterations);
}

}  // extern "C"
