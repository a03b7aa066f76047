// Particle and energy balance of LMEA models (include/fedm_hip.h, fedm_gd_balance_setup / fedm_gd_balance): the
// integrals the residual of gd.hip forms term by term, summed by kind -- contents, BDF2 rates of change, reaction totals,
// collision loss and Joule heating, the walls' facet integrals per tag, the ion flux, the induced current of a weighting
// potential, the Poisson rows over vertex groups, the field maximum and the nodal maxima -- from the resident state.
// diag.hip's pattern: a pass over the cells, one over the tagged facets (a workgroup owns a tag: its list is built at
// first use) and one over the vertices write slot-major partials, one workgroup reduces them; plain launches on the
// context's stream and one copy to the host.  Every sum and maximum has a fixed order (thread, wave by shuffles, the
// workgroup's waves one after the other, the partials) and nothing adds with floating-point atomics or waits for
// another workgroup, so a call is bitwise reproducible.  The point functions are gd_balance.hpp's value-only copies
// of gd.hip's; tests/test_gpu_balance.py holds their sums to the assembled residual.  The reductions' cores and the
// host's helpers are postproc.hpp's.
#include "gd_balance.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "postproc.hpp"
#include "solver.hpp"

namespace fedm {

// ---- the cells -------------------------------------------------------------------------------------
// A thread per cell (a stride loop beyond POST_BLOCKS workgroups).  The accumulators are indexed by compile-time
// numbers only (the species' loops are unrolled, the groups' to their maximum with a guard).
template <int NEQ>
__global__ __launch_bounds__(POST_THREADS) void gd_balance_cell_kernel(
    int nc, int nv, const fedm_gd_desc *__restrict__ md, const double *__restrict__ fields,
    const double *__restrict__ coords, const int *__restrict__ cells, const double *__restrict__ u,
    const double *__restrict__ uold, const double *__restrict__ uold1, double dt, double dt_old,
    const double *__restrict__ psi, const int8_t *__restrict__ group, int n_groups, double *__restrict__ sum_part,
    double *__restrict__ max_part, int *__restrict__ idx_part, int *__restrict__ flag_part) {
    constexpr int ns = NEQ - 1, IPHI = NEQ - 1, ie = ns - 1;
    const double two_pi = 6.283185307179586476925286766559;
    __shared__ double lds_sum[BAL_CELL_SUMS][POST_WAVES];
    __shared__ double lds_mv[1][POST_WAVES];
    __shared__ int lds_mi[1][POST_WAVES];
    const int nr = md->n_reactions, nq = md->n_qp;
    const bool groups = group && n_groups > 0;
    const double tr = dt / dt_old, trp1 = 1.0 + tr, tr2p1 = 1.0 + 2.0 * tr;
    // the reactions' running sums live in LDS, a column per thread: their loop stays rolled (unrolled to the
    // descriptor's 16 reactions the kernel wanted more than 512 registers: 360 spilled bytes a lane for five
    // equations), and a run-time reaction index into LDS costs nothing
    __shared__ double lds_reac[BAL_GR][POST_THREADS];
    double acc[BAL_CELL_SUMS];
#pragma unroll
    for (int k = 0; k < BAL_CELL_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < BAL_GR; ++j) lds_reac[j][threadIdx.x] = 0.0;
    MaxIdx mx[1] = {{-1.0, INT_MAX}};   // |E| >= 0: -1 stands for 'no cell'
    bool bad = false;
    for (int cell = blockIdx.x * blockDim.x + threadIdx.x; cell < nc; cell += gridDim.x * blockDim.x) {
        BalCell c;
        double U[3][NEQ];
        bad |= bal_load_cell<NEQ>(cell, md, coords, cells, u, c, U);
        double Uo[3][ns], Uo1[3][ns];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int e = 0; e < ns; ++e) {
                Uo[a][e] = uold[(size_t)c.v[a] * NEQ + e];
                Uo1[a][e] = uold1[(size_t)c.v[a] * NEQ + e];
            }
        double gP[2] = {0.0, 0.0}, mp[2] = {0.0, 0.0};   // grad Phi; -grad psi
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            gP[0] += U[a][IPHI] * c.G[a][0];
            gP[1] += U[a][IPHI] * c.G[a][1];
        }
        const double Em = sqrt(gP[0] * gP[0] + gP[1] * gP[1]);
        if (psi) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double pa = psi[c.v[a]];
                mp[0] -= pa * c.G[a][0];
                mp[1] -= pa * c.G[a][1];
            }
        }
        double chk = Em, rW = 0.0, rH[3] = {0.0, 0.0, 0.0};
        for (int q = 0; q < nq; ++q) {
            const double phi[3] = {1.0 - md->qp_x[q] - md->qp_y[q], md->qp_x[q], md->qp_y[q]};
            const double rq = c.rn[0] * phi[0] + c.rn[1] * phi[1] + c.rn[2] * phi[2];
            const double W = md->qp_w[q] * c.detJ * two_pi * rq;
            BalPoint<NEQ> p;
            bal_point<NEQ>(fields, nv, nr, c, U, phi, p);
            // contents and the BDF2 term, gd.hip's u_part and T
#pragma unroll
            for (int comp = 0; comp < ns; ++comp) {
                const double ulog = p.u[comp].v;
                double uo = 0.0, uo1 = 0.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    uo += Uo[a][comp] * phi[a];
                    uo1 += Uo1[a][comp] * phi[a];
                }
                const double u_part = (ulog * tr2p1 - (trp1 * trp1) * uo + (tr * tr) * uo1) * (1.0 / trp1);
                const double T = p.e[comp] * u_part * (1.0 / dt);
                acc[BAL_CONTENT + comp] += W * p.e[comp];
                acc[BAL_RATE + comp] += W * T;
                chk += T;
            }
            // reaction rates and the energy they take, Source_term / Energy_Source_term (functions.py:835-843, 901-912)
            double me_arg = 0.0, loss = 0.0;
            if (md->mean_energy_form == FEDM_GD_ME_UNKNOWN_RATIO) me_arg = p.u[0].v / p.u[ie].v;
#pragma unroll 1
            for (int j = 0; j < nr; ++j) {
                double rate = bal_rate_coefficient(fields, nv, ns, nr, j, c, phi, p.dme.v);
#pragma unroll
                for (int i = 0; i < ns; ++i)
                    for (int e = 0; e < md->power[j][i]; ++e) rate = (i == 0) ? rate * md->N0 : rate * p.e[i];
                lds_reac[j][threadIdx.x] += W * rate;
                const double lj = md->energy_loss[j];   // functions.py:905-911
                if (lj > 7e77 && lj < 8e77) loss += (md->energy_Ei - me_arg) * rate;
                else if (lj > 9e99 && lj < 1e100) loss += me_arg * rate;
                else loss += lj * rate;
            }
            acc[BAL_LOSS] += W * loss;
            // Joule heating, fedm-gd.py:359, and the induced current of the species' fluxes
            double gex, gey;
            bal_flux(md->sign[ie], p.u[ie], p.e[ie], p.D[ie], p.mu[ie], p.Ex, p.Ey, md->grad_diffusion[ie] != 0, gex, gey);
            const double joule = -(gex * p.Ex + gey * p.Ey);
            acc[BAL_JOULE] += W * joule;
            chk += loss + joule;
            if (psi) {
                double cur = 0.0;
#pragma unroll
                for (int s = 1; s < ns; ++s) {
                    double gx = gex, gy = gey;
                    if (s != ie) bal_species_flux<NEQ>(md, p, s, gx, gy);
                    cur += md->sign[s] * (gx * mp[0] + gy * mp[1]);
                }
                acc[BAL_CURRENT] += W * cur;
                chk += cur;
            }
            if (groups) {   // the Poisson row's charge part: -rho phi_a, rho = (e/eps0) sum_i sign_i n_i
                double h = 0.0;
#pragma unroll
                for (int i = 1; i < ns; ++i) h -= (md->sign[i] * md->charge_over_eps) * p.e[i];
                rW += W;
#pragma unroll
                for (int a = 0; a < 3; ++a) rH[a] += W * phi[a] * h;
            }
        }
        if (groups) {
            double R[3];
            int g[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                R[a] = (gP[0] * c.G[a][0] + gP[1] * c.G[a][1]) * rW + rH[a];
                chk += R[a];
                g[a] = group[c.v[a]];
            }
            if (g[0] | g[1] | g[2]) {
                // (compile-time slots: no run-time index into the accumulators; adding 0.0 changes no bit)
#pragma unroll
                for (int k = 0; k < FEDM_GD_BAL_MAX_GROUPS; ++k) {
                    if (k >= n_groups) continue;
#pragma unroll
                    for (int a = 0; a < 3; ++a) acc[BAL_GROUP0 + k] += g[a] == k + 1 ? R[a] : 0.0;
                }
            }
        }
        bad |= !isfinite(chk);
        mx[0].take(Em, cell);
    }
#pragma unroll
    for (int j = 0; j < BAL_GR; ++j) acc[BAL_REACTION + j] = lds_reac[j][threadIdx.x];
    const double s = block_sums(acc, lds_sum);
    const MaxIdx m = block_maxes(mx, lds_mv, lds_mi);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((int)threadIdx.x < BAL_CELL_SUMS) sum_part[(size_t)threadIdx.x * POST_BLOCKS + blockIdx.x] = s;
    if (threadIdx.x == 0) {
        max_part[blockIdx.x] = m.v;
        idx_part[blockIdx.x] = m.i;
        flag_part[blockIdx.x] = any_bad;
    }
}

// ---- the tagged facets -----------------------------------------------------------------------------
// Workgroup t owns tag t + 1 and walks its list; thread k the facets k, k + POST_THREADS, ...  The integrands are the
// facet block of gd_element: the accumulators are indexed by the component, never by the tag.
template <int NEQ>
__global__ __launch_bounds__(POST_THREADS) void gd_balance_facet_kernel(
    int nv, const fedm_gd_desc *__restrict__ md, const double *__restrict__ fields, const double *__restrict__ coords,
    const int *__restrict__ cells, const double *__restrict__ u, BalFacets facets, const int *__restrict__ list,
    double *__restrict__ facet_part, int *__restrict__ flag_part) {
    constexpr int ns = NEQ - 1, ie = ns - 1;
    const double two_pi = 6.283185307179586476925286766559;
    __shared__ double lds_sum[BAL_FACET_SUMS][POST_WAVES];
    const int tag = blockIdx.x + 1, nr = md->n_reactions;
    double acc[BAL_FACET_SUMS];
#pragma unroll
    for (int k = 0; k < BAL_FACET_SUMS; ++k) acc[k] = 0.0;
    bool bad = false;
    for (int f = facets.ptr[tag - 1] + (int)threadIdx.x; f < facets.ptr[tag]; f += blockDim.x) {
        const int cell = list[f] / 3, i = list[f] - 3 * cell;
        BalCell c;
        double U[3][NEQ];
        bad |= bal_load_cell<NEQ>(cell, md, coords, cells, u, c, U);
        const int j = (i == 0) ? 1 : 0, kk = (i == 2) ? 1 : 2;
        // (the corner's and the ends' entries by selection: a run-time index would send the cell to scratch)
        const double Gi0 = i == 0 ? c.G[0][0] : i == 1 ? c.G[1][0] : c.G[2][0];
        const double Gi1 = i == 0 ? c.G[0][1] : i == 1 ? c.G[1][1] : c.G[2][1];
        const double xj0 = j == 0 ? c.x[0][0] : c.x[1][0], xj1 = j == 0 ? c.x[0][1] : c.x[1][1];
        const double xk0 = kk == 1 ? c.x[1][0] : c.x[2][0], xk1 = kk == 1 ? c.x[1][1] : c.x[2][1];
        const double gi = sqrt(Gi0 * Gi0 + Gi1 * Gi1);
        const double nx = -Gi0 / gi, ny = -Gi1 / gi;
        const double ex = xj0 - xk0, ey = xj1 - xk1;
        const double L = sqrt(ex * ex + ey * ey);
        double chk = 0.0;
        for (int t = 0; t < md->n_fqp; ++t) {
            const double pj = 1.0 - md->fqp_t[t], pk = md->fqp_t[t];
            const double phi[3] = {j == 0 ? pj : 0.0, j == 1 ? pj : (kk == 1 ? pk : 0.0), kk == 2 ? pk : 0.0};
            const double rq = c.rn[0] * phi[0] + c.rn[1] * phi[1] + c.rn[2] * phi[2];
            const double W = md->fqp_w[t] * L * two_pi * rq;
            BalPoint<NEQ> p;
            bal_point<NEQ>(fields, nv, nr, c, U, phi, p);
            const double En = p.Ex * nx + p.Ey * ny;
            double ion = 0.0;   // Ion_flux = sum Max(Gamma_i . n, 0), fedm-gd.py:351
#pragma unroll
            for (int s = 1; s < ns; ++s) {
                if (!md->is_ion[s]) continue;
                double gx, gy;
                bal_flux(md->sign[s], p.u[s], p.e[s], p.D[s], p.mu[s], p.Ex, p.Ey, md->grad_diffusion[s] != 0, gx, gy);
                const double gn = gx * nx + gy * ny;
                ion = ion + (gn + fabs(gn)) * 0.5;
            }
            acc[BAL_GS] += W * ion;
            chk += ion;
            const double vth_e = sqrt(md->vth_e_coef * p.me);
#pragma unroll
            for (int comp = 0; comp < ns; ++comp) {
                const int sp = (comp == 0) ? ie : comp;
                const int et = md->eq_type[sp];
                if (et == FEDM_EQ_REACTION) continue;
                const double ref = md->ref[tag - 1][sp];
                const double fac = (1.0 - ref) / (1.0 + ref);
                double vth = (sp == ie) ? vth_e : md->vth[sp];
                double mu_scale = 1.0, gam = md->gamma[tag - 1];
                if (comp == 0) {   // energy: 5/3 mu, 1.3333 vth, gamma * mean energy of secondaries
                    vth = vth * 1.3333;
                    mu_scale = 5.0 / 3.0;
                    gam = gam * md->we_secondary;
                }
                const double dens = p.e[comp];
                double val;
                if (et == FEDM_EQ_DIFFUSION_REACTION) {
                    val = fac * (0.5 * vth * dens);
                } else {
                    val = fac * ((0.5 * vth + fabs((md->sign[sp] * mu_scale) * (p.mu[sp] * En))) * dens);
                    if (sp == ie) val = val - (2.0 * gam / (1.0 + ref)) * ion;
                }
                acc[comp] += W * val;
                chk += val;
            }
        }
        bad |= !isfinite(chk);
    }
    const double s = block_sums(acc, lds_sum);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((int)threadIdx.x < BAL_FACET_SUMS) facet_part[(size_t)threadIdx.x * FEDM_MAX_TAGS + blockIdx.x] = s;
    if (threadIdx.x == 0) flag_part[2 * POST_BLOCKS + blockIdx.x] = any_bad;
}

// ---- the vertices ----------------------------------------------------------------------------------
// A thread per vertex: the nodal maxima of the components below the potential and of u_0 - u_e (the log of the mean
// energy); every component is looked at for the flag.
template <int NEQ>
__global__ __launch_bounds__(POST_THREADS) void gd_balance_vertex_kernel(int nv, const double *__restrict__ u,
                                                                        double *__restrict__ max_part,
                                                                        int *__restrict__ idx_part,
                                                                        int *__restrict__ flag_part) {
    constexpr int ns = NEQ - 1, NM = ns + 1;
    __shared__ double lds_mv[NM][POST_WAVES];
    __shared__ int lds_mi[NM][POST_WAVES];
    MaxIdx mx[NM];
#pragma unroll
    for (int s = 0; s < NM; ++s) mx[s] = MaxIdx{-INFINITY, INT_MAX};
    bool bad = false;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += gridDim.x * blockDim.x) {
        double val[NEQ];
#pragma unroll
        for (int s = 0; s < NEQ; ++s) {
            val[s] = u[(size_t)v * NEQ + s];
            bad |= !isfinite(val[s]);
        }
#pragma unroll
        for (int s = 0; s < ns; ++s) mx[s].take(val[s], v);
        mx[ns].take(val[0] - val[ns - 1], v);
    }
    const MaxIdx m = block_maxes(mx, lds_mv, lds_mi);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((int)threadIdx.x < NM) {
        // (slot ns of this model goes to the last slot: the finish reads BAL_NODAL slots whatever the model)
        const int slot = (int)threadIdx.x == ns ? BAL_NODAL - 1 : (int)threadIdx.x;
        max_part[(size_t)(1 + slot) * POST_BLOCKS + blockIdx.x] = m.v;
        idx_part[(size_t)(1 + slot) * POST_BLOCKS + blockIdx.x] = m.i;
    }
    if (threadIdx.x == 0) flag_part[POST_BLOCKS + blockIdx.x] = any_bad;
}

// ---- second pass -----------------------------------------------------------------------------------
// One workgroup: thread t brings the partials of workgroup t (nbc of the cell pass, nbv of the vertex pass, both at
// most POST_BLOCKS = POST_THREADS), reduced slot by slot in the same fixed order; the tags' sums are final already.
// `ns`: the model's; the nodal slots ns .. BAL_NODAL - 2 were never written and are not read.
__global__ __launch_bounds__(POST_THREADS) void gd_balance_finish_kernel(
    int nbc, int nbv, int ns, const double *__restrict__ coords, const int *__restrict__ cells,
    const double *__restrict__ sum_part, const double *__restrict__ facet_part, const double *__restrict__ max_part,
    const int *__restrict__ idx_part, const int *__restrict__ flag_part, BalResult *__restrict__ res) {
    constexpr int NM = 1 + BAL_NODAL;
    __shared__ double lds_sum[BAL_CELL_SUMS][POST_WAVES];
    __shared__ double lds_mv[NM][POST_WAVES];
    __shared__ int lds_mi[NM][POST_WAVES];
    const int t = threadIdx.x;
    double sv[BAL_CELL_SUMS];
#pragma unroll
    for (int k = 0; k < BAL_CELL_SUMS; ++k) sv[k] = t < nbc ? sum_part[(size_t)k * POST_BLOCKS + t] : 0.0;
    MaxIdx mv[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        const bool used = k == 0 || k - 1 < ns || k == NM - 1;
        const bool have = used && t < (k == 0 ? nbc : nbv);
        mv[k].v = have ? max_part[(size_t)k * POST_BLOCKS + t] : -INFINITY;
        mv[k].i = have ? idx_part[(size_t)k * POST_BLOCKS + t] : INT_MAX;
    }
    const int bad = (t < nbc && flag_part[t]) || (t < nbv && flag_part[POST_BLOCKS + t]) ||
                    (t < FEDM_MAX_TAGS && flag_part[2 * POST_BLOCKS + t]);
    const double s = block_sums(sv, lds_sum);
    const MaxIdx m = block_maxes(mv, lds_mv, lds_mi);
    const int any_bad = __syncthreads_or(bad);
    if (t < BAL_CELL_SUMS) res->sum[t] = s;
    if (t < BAL_FACET_SUMS * FEDM_MAX_TAGS) (&res->facet[0][0])[t] = facet_part[t];
    const bool none = m.i == INT_MAX;
    if (t == 0) {
        res->field_max = none ? 0.0 : m.v;
        res->cell = none ? -1 : m.i;
        double cr = 0.0, cz = 0.0;
        if (!none) cell_centroid(coords, cells, m.i, cr, cz);
        res->centroid[0] = cr;
        res->centroid[1] = cz;
        res->not_finite = any_bad;
        res->pad_ = 0;
    } else if (t < NM) {
        res->nodal_max[t - 1] = none ? 0.0 : m.v;
        res->vertex[t - 1] = none ? -1 : m.i;
    }
}

// ---- host ------------------------------------------------------------------------------------------
void gd_balance_release(Ctx &c) {
    GdBalance *b = c.gd_balance;
    if (!b) return;
    void *ptrs[] = {b->psi, b->group, b->facet_list, b->sum_part, b->facet_part, b->max_part, b->idx_part, b->flag_part,
                    b->result};
    for (void *p : ptrs)
        if (p) hipFree(p);
    delete b;
    c.gd_balance = nullptr;
}

namespace {

int bal_check_ctx(const Ctx &c, const char *who) {
    if (c.model_kind != 1) return refuse(who, "an LFA context (the balance is the LMEA family's; fedm_diagnostics has the LFA observables)");
    if (c.n_owned != c.nv) return refuse(who, "a context with ghost vertices (one GPU only)");
    return 0;
}

// the buffers and the tags' facet lists, once per context
int ensure_balance(Ctx &c) {
    if (c.gd_balance) return 0;
    std::vector<int8_t> tags((size_t)3 * c.nc);
    if (c.nc && hipMemcpy(tags.data(), c.d_ftags, tags.size(), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("fedm_gd_balance: the facet tags could not be read");
        return -1;
    }
    GdBalance *b = new GdBalance();
    c.gd_balance = b;
    std::vector<int> list;
    for (int t = 1; t <= FEDM_MAX_TAGS; ++t) {   // by tag, then in ascending (cell, corner) order
        b->facets.ptr[t - 1] = (int)list.size();
        for (size_t k = 0; k < tags.size(); ++k)
            if (tags[k] == t) list.push_back((int)k);
    }
    b->facets.ptr[FEDM_MAX_TAGS] = (int)list.size();
    constexpr int NM = 1 + BAL_NODAL;
    bool ok = hipMalloc((void **)&b->sum_part, sizeof(double) * BAL_CELL_SUMS * POST_BLOCKS) == hipSuccess &&
              hipMalloc((void **)&b->facet_part, sizeof(double) * BAL_FACET_SUMS * FEDM_MAX_TAGS) == hipSuccess &&
              hipMalloc((void **)&b->max_part, sizeof(double) * NM * POST_BLOCKS) == hipSuccess &&
              hipMalloc((void **)&b->idx_part, sizeof(int) * NM * POST_BLOCKS) == hipSuccess &&
              hipMalloc((void **)&b->flag_part, sizeof(int) * (2 * POST_BLOCKS + FEDM_MAX_TAGS)) == hipSuccess &&
              hipMalloc((void **)&b->result, sizeof(BalResult)) == hipSuccess &&
              hipMalloc((void **)&b->facet_list, sizeof(int) * std::max<size_t>(list.size(), 1)) == hipSuccess;
    if (ok && !list.empty())
        ok = hipMemcpy(b->facet_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        gd_balance_release(c);
        set_error("fedm_gd_balance: out of device memory for the reductions' buffers");
        return -1;
    }
    return 0;
}

template <int NEQ>
void launch_balance(Ctx &c) {
    GdBalance &b = *c.gd_balance;
    const int nbc = std::max(std::min((c.nc + POST_THREADS - 1) / POST_THREADS, POST_BLOCKS), 1);
    const int nbv = std::max(std::min((c.nv + POST_THREADS - 1) / POST_THREADS, POST_BLOCKS), 1);
    const dim3 t(POST_THREADS);
    hipLaunchKernelGGL((gd_balance_cell_kernel<NEQ>), dim3(nbc), t, 0, c.stream, c.nc, c.nv, c.d_gd, c.d_gd_fields,
                       c.d_coords, c.d_cells, c.d_u, c.d_uold, c.d_uold1, c.dt, c.dt_old, b.psi, b.group, b.n_groups,
                       b.sum_part, b.max_part, b.idx_part, b.flag_part);
    hipLaunchKernelGGL((gd_balance_facet_kernel<NEQ>), dim3(FEDM_MAX_TAGS), t, 0, c.stream, c.nv, c.d_gd, c.d_gd_fields,
                       c.d_coords, c.d_cells, c.d_u, b.facets, b.facet_list, b.facet_part, b.flag_part);
    hipLaunchKernelGGL((gd_balance_vertex_kernel<NEQ>), dim3(nbv), t, 0, c.stream, c.nv, c.d_u, b.max_part, b.idx_part,
                       b.flag_part);
    hipLaunchKernelGGL(gd_balance_finish_kernel, dim3(1), t, 0, c.stream, nbc, nbv, NEQ - 1, c.d_coords, c.d_cells,
                       b.sum_part, b.facet_part, b.max_part, b.idx_part, b.flag_part, b.result);
}

}  // namespace
}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_gd_balance_setup(fedm_ctx *h, const double *psi, const int8_t *group, int n_groups) {
    const char *who = "fedm_gd_balance_setup";
    if (!h) return refuse(who, "null context");
    Ctx &c = h->c;
    if (const int rc = bal_check_ctx(c, who)) return rc;
    return weighting_setup(c, who, FEDM_GD_BAL_MAX_GROUPS, false, psi, group, n_groups, c.gd_balance, ensure_balance);
}

int fedm_gd_balance(fedm_ctx *h, struct fedm_gd_balance *out) {
    const char *who = "fedm_gd_balance";
    if (!h || !out) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (const int rc = bal_check_ctx(c, who)) return rc;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (const int rc = ensure_balance(c)) return rc;
    if (c.neq < 3 || c.neq > 6) return refuse(who, std::to_string(c.neq) + " equations: 3 to 6 are built");
    with_gd_neq(c, [&](auto neq) { launch_balance<decltype(neq)::value>(c); });
    BalResult r;
    if (const int rc = read_result(c, r, c.gd_balance->result)) return rc;
    const int ns = c.neq - 1, nr = c.gd.n_reactions;
    *out = {};
    for (int s = 0; s < ns; ++s) {
        out->content[s] = r.sum[BAL_CONTENT + s];
        out->rate_of_change[s] = r.sum[BAL_RATE + s];
        out->nodal_max[s] = r.nodal_max[s];
        out->nodal_max_vertex[s] = r.vertex[s];
    }
    out->nodal_max[ns] = r.nodal_max[BAL_NODAL - 1];
    out->nodal_max_vertex[ns] = r.vertex[BAL_NODAL - 1];
    for (int s = ns + 1; s < FEDM_GD_MAX_SPECIES + 1; ++s) out->nodal_max_vertex[s] = -1;
    for (int j = 0; j < nr; ++j) out->reaction[j] = r.sum[BAL_REACTION + j];
    out->collision_loss = r.sum[BAL_LOSS];
    out->joule = r.sum[BAL_JOULE];
    for (int t = 0; t < c.gd.n_tags; ++t) {
        for (int s = 0; s < ns; ++s) out->wall[t][s] = r.facet[s][t];
        out->ion_flux[t] = r.facet[BAL_GS][t];
    }
    out->induced_current = r.sum[BAL_CURRENT];
    for (int g = 0; g < c.gd_balance->n_groups; ++g) out->group_sum[g] = r.sum[BAL_GROUP0 + g];
    out->field_max = r.field_max;
    out->field_max_centroid[0] = r.centroid[0];
    out->field_max_centroid[1] = r.centroid[1];
    out->field_max_cell = r.cell;
    out->finite = r.not_finite ? 0 : 1;
    return 0;
}

}  // extern "C"
