// Discharge diagnostics (include/fedm_hip.h, fedm_diag_setup / fedm_diagnostics): species integrals, field maxima with
// their cells, nodal maxima with their vertices, the Poisson rows summed over vertex groups and the induced current of
// a weighting potential, from the resident state.  A pass over the cells and one over the vertices write slot-major
// partials, one workgroup reduces them; plain launches on the context's stream and one copy to the host.  Every sum
// and maximum has a fixed order (thread, wave by shuffles, the workgroup's waves one after the other, the partials)
// and nothing adds with floating-point atomics, so a call is bitwise reproducible -- photo.hip's pattern.  The
// reductions' cores and the host's helpers are postproc.hpp's, one copy for every pass of this kind.
#include "diag.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

#include "element.hpp"
#include "postproc.hpp"
#include "solver.hpp"

namespace fedm {

struct DiagWindow {
    double r_lo, r_hi, z_lo, z_hi;
};

// ---- the cells -------------------------------------------------------------------------------------
// A thread per cell (a stride loop beyond POST_BLOCKS workgroups).  |E| and the coefficients once per cell as
// Element::setup has them, the densities at the model's quadrature points with Element::point's weight.  A cell with a
// ghost vertex (n_owned < nv) weighs its integrals' terms by the owned basis functions' sum; a cell without one by
// exactly 1.0.  The Poisson rows are the rows the assembly forms before dirichlet_kernel overwrites them: whole rows,
// taken for the owned group vertices.
template <int NS, bool PO, bool TAB>
__global__ __launch_bounds__(POST_THREADS) void diag_cell_kernel(
    int nc, int n_owned, const fedm_model_desc *__restrict__ md, const double *__restrict__ coords,
    const int *__restrict__ cells, const double *__restrict__ u, const double *__restrict__ psi,
    const int8_t *__restrict__ group, int n_groups, DiagWindow win, double *__restrict__ sum_part,
    double *__restrict__ max_part, int *__restrict__ idx_part, int *__restrict__ flag_part) {
    constexpr int NEQ = NS + (PO ? 1 : 0);
    const double two_pi = 6.283185307179586476925286766559;
    __shared__ double lds_sum[DIAG_SUMS][POST_WAVES];
    __shared__ double lds_mv[DIAG_CELL_MAXES][POST_WAVES];
    __shared__ int lds_mi[DIAG_CELL_MAXES][POST_WAVES];
    const bool axi = md->axisymmetric != 0, lin = md->linear_representation != 0;
    const bool groups = PO && group && n_groups > 0;
    const int nq = md->n_qp;
    double acc[DIAG_SUMS];
#pragma unroll
    for (int k = 0; k < DIAG_SUMS; ++k) acc[k] = 0.0;
    MaxIdx mx[DIAG_CELL_MAXES] = {{-1.0, INT_MAX}, {-1.0, INT_MAX}};   // |E| >= 0: -1 stands for 'no cell'
    bool bad = false;
    for (int cell = blockIdx.x * blockDim.x + threadIdx.x; cell < nc; cell += gridDim.x * blockDim.x) {
        int v[3];
        double x[3][2], U[3][NEQ];
        bool own[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[a] = cells[3 * (size_t)cell + a];
            own[a] = v[a] < n_owned;
            x[a][0] = coords[2 * (size_t)v[a]];
            x[a][1] = coords[2 * (size_t)v[a] + 1];
#pragma unroll
            for (int e = 0; e < NEQ; ++e) {
                U[a][e] = u[(size_t)v[a] * NEQ + e];
                bad |= !isfinite(U[a][e]);
            }
        }
        const bool all_owned = own[0] && own[1] && own[2], any_owned = own[0] || own[1] || own[2];
        CellGeom cg;
        cg.init(x, axi);
        double gP[2] = {0.0, 0.0}, Em = 1.0, invEm = 1.0;
        if (PO) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                gP[0] += U[a][NEQ - 1] * cg.G[a][0];
                gP[1] += U[a][NEQ - 1] * cg.G[a][1];
            }
            Em = sqrt(gP[0] * gP[0] + gP[1] * gP[1]);
            invEm = 1.0 / Em;
        }
        // the flux of species s dotted with -grad(psi): logarithmic n_s velp[s]; linear difp[s] + drfp[s] u_s
        double velp[NS], difp[NS], drfp[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) velp[s] = difp[s] = drfp[s] = 0.0;
        if (psi) {
            const double lnE = log(Em);
            double mp[2] = {0.0, 0.0};   // -grad(psi)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double pa = psi[v[a]];
                bad |= !isfinite(pa);
                mp[0] -= pa * cg.G[a][0];
                mp[1] -= pa * cg.G[a][1];
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int et = md->eq_type[s];
                if (et == FEDM_EQ_REACTION) continue;
                double Dv, Dd, gu[2] = {0.0, 0.0}, w[2] = {0.0, 0.0};
                termsum_eval<TAB>(md, md->D[s], Em, invEm, lnE, Dv, Dd);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    gu[0] += U[a][s] * cg.G[a][0];
                    gu[1] += U[a][s] * cg.G[a][1];
                }
                if (et == FEDM_EQ_DRIFT_DIFFUSION_REACTION) {
                    if (md->has_drift_w[s]) {
                        w[0] = md->drift_w[s][0];
                        w[1] = md->drift_w[s][1];
                    } else if (PO) {
                        double muv, mud;
                        termsum_eval<TAB>(md, md->mu[s], Em, invEm, lnE, muv, mud);
                        w[0] = -md->Z[s] * muv * gP[0];
                        w[1] = -md->Z[s] * muv * gP[1];
                    }
                }
                difp[s] = -Dv * (gu[0] * mp[0] + gu[1] * mp[1]);
                drfp[s] = w[0] * mp[0] + w[1] * mp[1];
                velp[s] = difp[s] + drfp[s];
            }
        }
        // quadrature: sum W om, sum W om n_s; for the rows sum W and sum W phi_a rho, rho = -(e/eps0) sum_s Z_s n_s
        double cW = 0.0, cN[NS], rW = 0.0, rH[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < NS; ++s) cN[s] = 0.0;
        for (int q = 0; q < nq; ++q) {
            const double xq = md->qp_x[q], yq = md->qp_y[q];
            const double phi[3] = {1.0 - xq - yq, xq, yq};
            const double rq = cg.rn[0] * phi[0] + cg.rn[1] * phi[1] + cg.rn[2] * phi[2];
            const double W = md->qp_w[q] * cg.detJ * two_pi * rq;
            const double om = all_owned ? 1.0
                                        : (own[0] ? phi[0] : 0.0) + (own[1] ? phi[1] : 0.0) + (own[2] ? phi[2] : 0.0);
            const double Wo = W * om;
            double h = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double us = U[0][s] * phi[0] + U[1][s] * phi[1] + U[2][s] * phi[2];
                const double n = lin ? us : exp(us);
                cN[s] += Wo * n;
                h -= md->Z[s] * n * md->charge_over_eps;
            }
            cW += Wo;
            if (groups) {
                rW += W;
#pragma unroll
                for (int a = 0; a < 3; ++a) rH[a] += W * phi[a] * h;
            }
        }
        double chk = PO ? Em : 0.0, cur = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            acc[s] += cN[s];
            chk += cN[s];
            cur += md->Z[s] * (lin ? difp[s] * cW + drfp[s] * cN[s] : velp[s] * cN[s]);
        }
        acc[DIAG_SUM_CURRENT] += cur;
        chk += cur;
        if (groups) {
            double R[3];
            int g[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                R[a] = (gP[0] * cg.G[a][0] + gP[1] * cg.G[a][1]) * rW + rH[a];
                chk += R[a];
                g[a] = own[a] ? group[v[a]] : 0;
            }
            if (g[0] | g[1] | g[2]) {
                // (compile-time slots: no run-time index into the accumulators; adding 0.0 changes no bit)
#pragma unroll
                for (int k = 0; k < FEDM_DIAG_MAX_GROUPS; ++k) {
                    if (k >= n_groups) break;
#pragma unroll
                    for (int a = 0; a < 3; ++a) acc[DIAG_SUM_GROUP0 + k] += g[a] == k + 1 ? R[a] : 0.0;
                }
            }
        }
        bad |= !isfinite(chk);
        if (PO && any_owned) {
            mx[0].take(Em, cell);
            const double cr = (x[0][0] + x[1][0] + x[2][0]) / 3.0, cz = (x[0][1] + x[1][1] + x[2][1]) / 3.0;
            if (cr >= win.r_lo && cr <= win.r_hi && cz >= win.z_lo && cz <= win.z_hi) mx[1].take(Em, cell);
        }
    }
    const double s = block_sums(acc, lds_sum);
    const MaxIdx m = block_maxes(mx, lds_mv, lds_mi);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((int)threadIdx.x < DIAG_SUMS) sum_part[(size_t)threadIdx.x * POST_BLOCKS + blockIdx.x] = s;
    if ((int)threadIdx.x < DIAG_CELL_MAXES) {
        max_part[(size_t)threadIdx.x * POST_BLOCKS + blockIdx.x] = m.v;
        idx_part[(size_t)threadIdx.x * POST_BLOCKS + blockIdx.x] = m.i;
    }
    if (threadIdx.x == 0) flag_part[blockIdx.x] = any_bad;
}

// ---- the vertices ----------------------------------------------------------------------------------
// A thread per owned vertex: the species' nodal maxima; every component is looked at for the flag.
__global__ __launch_bounds__(POST_THREADS) void diag_vertex_kernel(int n_owned, int ns, int neq,
                                                                   const double *__restrict__ u,
                                                                   double *__restrict__ max_part,
                                                                   int *__restrict__ idx_part,
                                                                   int *__restrict__ flag_part) {
    __shared__ double lds_mv[FEDM_MAX_SPECIES][POST_WAVES];
    __shared__ int lds_mi[FEDM_MAX_SPECIES][POST_WAVES];
    MaxIdx mx[FEDM_MAX_SPECIES];
#pragma unroll
    for (int s = 0; s < FEDM_MAX_SPECIES; ++s) mx[s] = MaxIdx{-INFINITY, INT_MAX};
    bool bad = false;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n_owned; v += gridDim.x * blockDim.x) {
#pragma unroll
        for (int s = 0; s < FEDM_MAX_SPECIES; ++s) {
            if (s >= ns) break;
            const double val = u[(size_t)v * neq + s];
            bad |= !isfinite(val);
            mx[s].take(val, v);
        }
        if (neq > ns) bad |= !isfinite(u[(size_t)v * neq + ns]);
    }
    const MaxIdx m = block_maxes(mx, lds_mv, lds_mi);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((int)threadIdx.x < FEDM_MAX_SPECIES) {
        max_part[(size_t)(DIAG_CELL_MAXES + threadIdx.x) * POST_BLOCKS + blockIdx.x] = m.v;
        idx_part[(size_t)(DIAG_CELL_MAXES + threadIdx.x) * POST_BLOCKS + blockIdx.x] = m.i;
    }
    if (threadIdx.x == 0) flag_part[POST_BLOCKS + blockIdx.x] = any_bad;
}

// ---- second pass -----------------------------------------------------------------------------------
// One workgroup: thread t brings the partials of workgroup t (nbc of the cell pass, nbv of the vertex pass, both at
// most POST_BLOCKS = POST_THREADS), reduced slot by slot in the same fixed order.
__global__ __launch_bounds__(POST_THREADS) void diag_finish_kernel(int nbc, int nbv, const double *__restrict__ coords,
                                                                   const int *__restrict__ cells,
                                                                   const double *__restrict__ sum_part,
                                                                   const double *__restrict__ max_part,
                                                                   const int *__restrict__ idx_part,
                                                                   const int *__restrict__ flag_part,
                                                                   DiagResult *__restrict__ res) {
    __shared__ double lds_sum[DIAG_SUMS][POST_WAVES];
    __shared__ double lds_mv[DIAG_CELL_MAXES + FEDM_MAX_SPECIES][POST_WAVES];
    __shared__ int lds_mi[DIAG_CELL_MAXES + FEDM_MAX_SPECIES][POST_WAVES];
    const int t = threadIdx.x;
    double sv[DIAG_SUMS];
#pragma unroll
    for (int k = 0; k < DIAG_SUMS; ++k) sv[k] = t < nbc ? sum_part[(size_t)k * POST_BLOCKS + t] : 0.0;
    MaxIdx mv[DIAG_CELL_MAXES + FEDM_MAX_SPECIES];
#pragma unroll
    for (int k = 0; k < DIAG_CELL_MAXES + FEDM_MAX_SPECIES; ++k) {
        const bool have = t < (k < DIAG_CELL_MAXES ? nbc : nbv);
        mv[k].v = have ? max_part[(size_t)k * POST_BLOCKS + t] : -INFINITY;
        mv[k].i = have ? idx_part[(size_t)k * POST_BLOCKS + t] : INT_MAX;
    }
    const int bad = (t < nbc && flag_part[t]) || (t < nbv && flag_part[POST_BLOCKS + t]);
    const double s = block_sums(sv, lds_sum);
    const MaxIdx m = block_maxes(mv, lds_mv, lds_mi);
    const int any_bad = __syncthreads_or(bad);
    if (t < DIAG_SUMS) res->sum[t] = s;
    if (t < DIAG_CELL_MAXES) {
        const bool none = m.i == INT_MAX;
        res->cell_max[t] = none ? 0.0 : m.v;
        res->cell[t] = none ? -1 : m.i;
        double cr = 0.0, cz = 0.0;
        if (!none) cell_centroid(coords, cells, m.i, cr, cz);
        res->centroid[t][0] = cr;
        res->centroid[t][1] = cz;
    } else if (t < DIAG_CELL_MAXES + FEDM_MAX_SPECIES) {
        const bool none = m.i == INT_MAX;
        res->nodal_max[t - DIAG_CELL_MAXES] = none ? 0.0 : m.v;
        res->vertex[t - DIAG_CELL_MAXES] = none ? -1 : m.i;
    }
    if (t == 0) {
        res->not_finite = any_bad;
        res->pad_ = 0;
    }
}

// ---- host ------------------------------------------------------------------------------------------
void diag_release(Ctx &c) {
    Diag *d = c.diag;
    if (!d) return;
    void *ptrs[] = {d->psi, d->group, d->sum_part, d->max_part, d->idx_part, d->flag_part, d->result};
    for (void *p : ptrs)
        if (p) hipFree(p);
    delete d;
    c.diag = nullptr;
}

namespace {

// the contexts the kernels are instantiated for (0), or the refusal
int check_ctx(const Ctx &c, const char *who) {
    if (c.model_kind != 0) return refuse(who, "the LMEA family has no diagnostics (LFA models only)");
    if (!c.poisson && c.ns > 2)
        return refuse(who, std::to_string(c.ns) + " species without a Poisson equation: at most 2 are built");
    return 0;
}

int ensure_diag(Ctx &c) {
    if (c.diag) return 0;
    Diag *d = new Diag();
    c.diag = d;
    constexpr int NMAX = DIAG_CELL_MAXES + FEDM_MAX_SPECIES;
    if (hipMalloc((void **)&d->sum_part, sizeof(double) * DIAG_SUMS * POST_BLOCKS) != hipSuccess ||
        hipMalloc((void **)&d->max_part, sizeof(double) * NMAX * POST_BLOCKS) != hipSuccess ||
        hipMalloc((void **)&d->idx_part, sizeof(int) * NMAX * POST_BLOCKS) != hipSuccess ||
        hipMalloc((void **)&d->flag_part, sizeof(int) * 2 * POST_BLOCKS) != hipSuccess ||
        hipMalloc((void **)&d->result, sizeof(DiagResult)) != hipSuccess) {
        diag_release(c);
        set_error("fedm_diagnostics: out of device memory for the reductions' buffers");
        return -1;
    }
    return 0;
}

void launch_diagnostics(Ctx &c, const double *u, const DiagWindow &win) {
    Diag &d = *c.diag;
    const int nbc = std::min((c.nc + POST_THREADS - 1) / POST_THREADS, POST_BLOCKS);
    const int nbv = std::max(std::min((c.n_owned + POST_THREADS - 1) / POST_THREADS, POST_BLOCKS), 1);
    const dim3 b(POST_THREADS);
    with_model_flags(c, [&](auto ns, auto po, auto tab) {
        constexpr int NS = decltype(ns)::value;
        constexpr bool PO = decltype(po)::value, TAB = decltype(tab)::value;
        hipLaunchKernelGGL((diag_cell_kernel<NS, PO, TAB>), dim3(nbc), b, 0, c.stream, c.nc, c.n_owned, c.d_model,
                           c.d_coords, c.d_cells, u, d.psi, d.group, d.n_groups, win, d.sum_part, d.max_part,
                           d.idx_part, d.flag_part);
    });
    hipLaunchKernelGGL(diag_vertex_kernel, dim3(nbv), b, 0, c.stream, c.n_owned, c.ns, c.neq, u, d.max_part, d.idx_part,
                       d.flag_part);
    hipLaunchKernelGGL(diag_finish_kernel, dim3(1), b, 0, c.stream, nbc, nbv, c.d_coords, c.d_cells, d.sum_part,
                       d.max_part, d.idx_part, d.flag_part, d.result);
}

}  // namespace
}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_diag_setup(fedm_ctx *h, const double *psi, const int8_t *group, int n_groups) {
    const char *who = "fedm_diag_setup";
    if (!h) return refuse(who, "null context");
    Ctx &c = h->c;
    if (const int rc = check_ctx(c, who)) return rc;
    return weighting_setup(c, who, FEDM_DIAG_MAX_GROUPS, true, psi, group, n_groups, c.diag, ensure_diag);
}

int fedm_diagnostics(fedm_ctx *h, const fedm_diag_opts *opts, fedm_diag *out) {
    const char *who = "fedm_diagnostics";
    if (!h || !opts || !out) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (const int rc = check_ctx(c, who)) return rc;
    if (opts->state != 0 && opts->state != 1)
        return refuse(who, "state " + std::to_string(opts->state) + ": 0 (u_new) or 1 (u_old)");
    if (std::isnan(opts->r_lo) || std::isnan(opts->r_hi) || std::isnan(opts->z_lo) || std::isnan(opts->z_hi))
        return refuse(who, "a window bound is NaN");
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (const int rc = ensure_diag(c)) return rc;
    if (opts->state == 0 && c.halo_pending) {   // (several GPUs: the ghost entries of u_new are exchanged lazily)
        comm_halo(c, c.d_u);
        c.halo_pending = false;
    }
    launch_diagnostics(c, opts->state == 0 ? c.d_u : c.d_uold, DiagWindow{opts->r_lo, opts->r_hi, opts->z_lo, opts->z_hi});
    DiagResult r;
    if (const int rc = read_result(c, r, c.diag->result)) return rc;
    *out = fedm_diag{};
    for (int s = 0; s < c.ns; ++s) {
        out->species_integral[s] = r.sum[s];
        out->nodal_max[s] = r.nodal_max[s];
        out->nodal_max_vertex[s] = r.vertex[s];
    }
    for (int s = c.ns; s < FEDM_MAX_SPECIES; ++s) out->nodal_max_vertex[s] = -1;
    for (int g = 0; g < c.diag->n_groups; ++g) out->group_sum[g] = r.sum[DIAG_SUM_GROUP0 + g];
    out->induced_current = r.sum[DIAG_SUM_CURRENT];
    out->field_max = r.cell_max[0];
    out->field_max_cell = r.cell[0];
    out->window_max = r.cell_max[1];
    out->window_max_cell = r.cell[1];
    for (int k = 0; k < 2; ++k) {
        out->field_max_centroid[k] = r.centroid[0][k];
        out->window_max_centroid[k] = r.centroid[1][k];
    }
    out->finite = r.not_finite ? 0 : 1;
    return 0;
}

}  // extern "C"
