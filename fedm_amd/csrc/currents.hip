// Electrode currents (include/fedm_hip.h, fedm_currents_setup / fedm_currents_solve / fedm_currents): the Shockley-Ramo
// currents of up to eight weighting potentials at once -- conduction, displacement, the coupling integral and the
// induced charge -- and their capacitance matrix, from the resident state of either family; the potentials themselves
// solved for on the device.  diag.hip's pattern: a pass over the cells writes slot-major partials, one workgroup
// reduces them; plain launches on the context's stream and one copy to the host.  Every sum has a fixed order (thread,
// wave by shuffles, the workgroup's waves one after the other, the partials) and nothing adds with floating-point
// atomics, so a call is bitwise reproducible.  The reductions' cores and the host's helpers are postproc.hpp's.
// A cell's part does not depend on the potential: sum W, the charge-weighted flux J = sum_s Z_s sum W Gamma_s (the
// gradients of P1 functions are constant on a cell, so Gamma_s . grad psi sums to J . grad psi), the charge moments
// Q_a = sum_s Z_s sum W n_s phi_a and the gradients of Phi and of D_t Phi.  It is formed once per cell, as
// diag_cell_kernel (LFA) or bal_point / bal_species_flux (LMEA) form it; each potential then costs three loads, its
// gradient and four sums (cur_accumulate).
#include "currents.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#include "element.hpp"
#include "gd_balance.hpp"
#include "postproc.hpp"
#include "solver.hpp"

namespace fedm {

// ---- what the families share -------------------------------------------------------------------------
// the variable-step BDF2 quotient of a nodal value (element.hpp, step_coef; gd_balance's rate_of_change)
__device__ __forceinline__ double cur_rate(double un, double uo, double uo1, double tr, double inv_dt) {
    const double trp1 = 1.0 + tr, tr2p1 = 1.0 + 2.0 * tr;
    return (un * tr2p1 - (trp1 * trp1) * uo + (tr * tr) * uo1) * (1.0 / trp1) * inv_dt;
}

struct CurCell {
    double cW;              // sum_q W
    double J[2];            // sum_s Z_s sum_q W Gamma_s
    double Q[3];            // sum_s Z_s sum_q W n_s phi_a
    double gP[2], gD[2];    // grad Phi(u_new), grad D_t Phi
};

// the potentials' sums of one cell; returns their sum for the not-finite flag.  Compile-time slots: no run-time index
// into the accumulators (diag_cell_kernel's groups)
__device__ __forceinline__ double cur_accumulate(double (&acc)[CUR_SUMS], const CurCell &cc, const double G[3][2],
                                                 const int v[3], const double *__restrict__ psi, int nvp, int n_psi) {
    double chk = 0.0;
#pragma unroll
    for (int k = 0; k < CUR_MAX; ++k) {
        if (k >= n_psi) break;
        const double *pk = psi + (size_t)k * nvp;
        const double p0 = pk[v[0]], p1 = pk[v[1]], p2 = pk[v[2]];
        double gp[2];
        cur_grad(G, p0, p1, p2, gp);
        const double cond = -(cc.J[0] * gp[0] + cc.J[1] * gp[1]);
        const double disp = cur_grad_dot(cc.cW, cc.gD, gp), coup = cur_grad_dot(cc.cW, cc.gP, gp);
        const double chg = p0 * cc.Q[0] + p1 * cc.Q[1] + p2 * cc.Q[2];
        acc[CUR_COND + k] += cond;
        acc[CUR_DISP + k] += disp;
        acc[CUR_COUP + k] += coup;
        acc[CUR_CHARGE + k] += chg;
        chk += (cond + disp) + (coup + chg);
    }
    return chk;
}

// ---- the cells, LFA ----------------------------------------------------------------------------------
// A thread per cell (a stride loop beyond POST_BLOCKS workgroups).  |E| and the coefficients once per cell as
// Element::setup has them, the densities at the model's quadrature points with Element::point's weight: the fluxes are
// diag_cell_kernel's, kept as vectors.
template <int NS, bool TAB>
__global__ __launch_bounds__(POST_THREADS) void currents_cell_kernel(
    int nc, int nvp, const fedm_model_desc *__restrict__ md, const double *__restrict__ coords,
    const int *__restrict__ cells, const double *__restrict__ u, const double *__restrict__ uold,
    const double *__restrict__ uold1, double dt, double dt_old, const double *__restrict__ psi, int n_psi,
    double *__restrict__ sum_part, int *__restrict__ flag_part) {
    constexpr int NEQ = NS + 1, IPHI = NS;
    const double two_pi = 6.283185307179586476925286766559;
    const bool axi = md->axisymmetric != 0, lin = md->linear_representation != 0;
    const int nq = md->n_qp;
    const double tr = dt / dt_old, inv_dt = 1.0 / dt;
    double acc[CUR_SUMS];
#pragma unroll
    for (int k = 0; k < CUR_SUMS; ++k) acc[k] = 0.0;
    bool bad = false;
    for (int cell = blockIdx.x * blockDim.x + threadIdx.x; cell < nc; cell += gridDim.x * blockDim.x) {
        int v[3];
        double x[3][2], U[3][NEQ], Dt[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[a] = cells[3 * (size_t)cell + a];
            x[a][0] = coords[2 * (size_t)v[a]];
            x[a][1] = coords[2 * (size_t)v[a] + 1];
#pragma unroll
            for (int e = 0; e < NEQ; ++e) {
                U[a][e] = u[(size_t)v[a] * NEQ + e];
                bad |= !isfinite(U[a][e]);
            }
            Dt[a] = cur_rate(U[a][IPHI], uold[(size_t)v[a] * NEQ + IPHI], uold1[(size_t)v[a] * NEQ + IPHI], tr, inv_dt);
        }
        CellGeom cg;
        cg.init(x, axi);
        CurCell cc;
        cur_grad(cg.G, U[0][IPHI], U[1][IPHI], U[2][IPHI], cc.gP);
        cur_grad(cg.G, Dt[0], Dt[1], Dt[2], cc.gD);
        const double Em = sqrt(cc.gP[0] * cc.gP[0] + cc.gP[1] * cc.gP[1]), invEm = 1.0 / Em, lnE = log(Em);
        // the flux of species s: logarithmic n_s vel[s]; linear dif[s] + drf[s] u_s
        double dif[NS][2], drf[NS][2];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            dif[s][0] = dif[s][1] = drf[s][0] = drf[s][1] = 0.0;
            const int et = md->eq_type[s];
            if (et == FEDM_EQ_REACTION) continue;
            double Dv, Dd, gu[2];
            termsum_eval<TAB>(md, md->D[s], Em, invEm, lnE, Dv, Dd);
            cur_grad(cg.G, U[0][s], U[1][s], U[2][s], gu);
            if (et == FEDM_EQ_DRIFT_DIFFUSION_REACTION) {
                if (md->has_drift_w[s]) {
                    drf[s][0] = md->drift_w[s][0];
                    drf[s][1] = md->drift_w[s][1];
                } else {
                    double muv, mud;
                    termsum_eval<TAB>(md, md->mu[s], Em, invEm, lnE, muv, mud);
                    drf[s][0] = -md->Z[s] * muv * cc.gP[0];
                    drf[s][1] = -md->Z[s] * muv * cc.gP[1];
                }
            }
            dif[s][0] = -Dv * gu[0];
            dif[s][1] = -Dv * gu[1];
        }
        double cW = 0.0, cN[NS];
        cc.Q[0] = cc.Q[1] = cc.Q[2] = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) cN[s] = 0.0;
        for (int q = 0; q < nq; ++q) {
            const double xq = md->qp_x[q], yq = md->qp_y[q];
            const double phi[3] = {1.0 - xq - yq, xq, yq};
            const double rq = cg.rn[0] * phi[0] + cg.rn[1] * phi[1] + cg.rn[2] * phi[2];
            const double W = md->qp_w[q] * cg.detJ * two_pi * rq;
            double rho = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double us = U[0][s] * phi[0] + U[1][s] * phi[1] + U[2][s] * phi[2];
                const double n = lin ? us : exp(us);
                cN[s] += W * n;
                rho += md->Z[s] * n;
            }
            cW += W;
#pragma unroll
            for (int a = 0; a < 3; ++a) cc.Q[a] += W * phi[a] * rho;
        }
        cc.cW = cW;
        cc.J[0] = cc.J[1] = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int d = 0; d < 2; ++d)
                cc.J[d] += md->Z[s] * (lin ? dif[s][d] * cW + drf[s][d] * cN[s] : (dif[s][d] + drf[s][d]) * cN[s]);
        }
        const double chk = cur_accumulate(acc, cc, cg.G, v, psi, nvp, n_psi);
        bad |= !isfinite(chk + Em + (cc.J[0] + cc.J[1]) + (cc.gD[0] + cc.gD[1]));
    }
    cur_write_partials(acc, bad, sum_part, flag_part);
}

// ---- the cells, LMEA ---------------------------------------------------------------------------------
// The residual's own fluxes of the current step at every quadrature point (gd_balance.hpp: bal_point, bal_species_flux;
// the electrons' by bal_flux, as gd_balance_cell_kernel takes them), species s >= 1 with sign_s.
template <int NEQ>
__global__ __launch_bounds__(POST_THREADS) void gd_currents_cell_kernel(
    int nc, int nv, int nvp, const fedm_gd_desc *__restrict__ md, const double *__restrict__ fields,
    const double *__restrict__ coords, const int *__restrict__ cells, const double *__restrict__ u,
    const double *__restrict__ uold, const double *__restrict__ uold1, double dt, double dt_old,
    const double *__restrict__ psi, int n_psi, double *__restrict__ sum_part, int *__restrict__ flag_part) {
    constexpr int ns = NEQ - 1, IPHI = NEQ - 1, ie = ns - 1;
    const double two_pi = 6.283185307179586476925286766559;
    const int nr = md->n_reactions, nq = md->n_qp;
    const double tr = dt / dt_old, inv_dt = 1.0 / dt;
    double acc[CUR_SUMS];
#pragma unroll
    for (int k = 0; k < CUR_SUMS; ++k) acc[k] = 0.0;
    bool bad = false;
    for (int cell = blockIdx.x * blockDim.x + threadIdx.x; cell < nc; cell += gridDim.x * blockDim.x) {
        BalCell c;
        double U[3][NEQ], Dt[3];
        bad |= bal_load_cell<NEQ>(cell, md, coords, cells, u, c, U);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            Dt[a] = cur_rate(U[a][IPHI], uold[(size_t)c.v[a] * NEQ + IPHI], uold1[(size_t)c.v[a] * NEQ + IPHI], tr, inv_dt);
        CurCell cc;
        cur_grad(c.G, U[0][IPHI], U[1][IPHI], U[2][IPHI], cc.gP);
        cur_grad(c.G, Dt[0], Dt[1], Dt[2], cc.gD);
        cc.cW = 0.0;
        cc.J[0] = cc.J[1] = 0.0;
        cc.Q[0] = cc.Q[1] = cc.Q[2] = 0.0;
        for (int q = 0; q < nq; ++q) {
            const double phi[3] = {1.0 - md->qp_x[q] - md->qp_y[q], md->qp_x[q], md->qp_y[q]};
            const double rq = c.rn[0] * phi[0] + c.rn[1] * phi[1] + c.rn[2] * phi[2];
            const double W = md->qp_w[q] * c.detJ * two_pi * rq;
            BalPoint<NEQ> p;
            bal_point<NEQ>(fields, nv, nr, c, U, phi, p);
            double jx = 0.0, jy = 0.0, rho = 0.0;
#pragma unroll
            for (int s = 1; s < ns; ++s) {
                double gx, gy;
                if (s == ie)
                    bal_flux(md->sign[ie], p.u[ie], p.e[ie], p.D[ie], p.mu[ie], p.Ex, p.Ey, md->grad_diffusion[ie] != 0, gx, gy);
                else
                    bal_species_flux<NEQ>(md, p, s, gx, gy);
                jx += md->sign[s] * gx;
                jy += md->sign[s] * gy;
                rho += md->sign[s] * p.e[s];
            }
            cc.cW += W;
            cc.J[0] += W * jx;
            cc.J[1] += W * jy;
#pragma unroll
            for (int a = 0; a < 3; ++a) cc.Q[a] += W * phi[a] * rho;
        }
        const double chk = cur_accumulate(acc, cc, c.G, c.v, psi, nvp, n_psi);
        bad |= !isfinite(chk + (cc.gP[0] + cc.gP[1]) + (cc.J[0] + cc.J[1]) + (cc.gD[0] + cc.gD[1]));
    }
    cur_write_partials(acc, bad, sum_part, flag_part);
}

// ---- the capacitance ---------------------------------------------------------------------------------
// Column h: sum W grad psi_g . grad psi_h for g <= h by cur_grad_dot, the function of the displacement with psi_h in
// place of D_t Phi; the host writes [g][h] and [h][g] from the one sum.  Desc: either family's descriptor (the
// quadrature rule and the symmetry are all it gives).
template <class Desc>
__global__ __launch_bounds__(POST_THREADS) void currents_capacitance_kernel(
    int nc, int nvp, const Desc *__restrict__ md, const double *__restrict__ coords, const int *__restrict__ cells,
    const double *__restrict__ psi, int h, double *__restrict__ sum_part, int *__restrict__ flag_part) {
    const double two_pi = 6.283185307179586476925286766559;
    const bool axi = md->axisymmetric != 0;
    const int nq = md->n_qp;
    double acc[CUR_MAX];
#pragma unroll
    for (int k = 0; k < CUR_MAX; ++k) acc[k] = 0.0;
    bool bad = false;
    for (int cell = blockIdx.x * blockDim.x + threadIdx.x; cell < nc; cell += gridDim.x * blockDim.x) {
        BalCell c;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c.v[a] = cells[3 * (size_t)cell + a];
            c.x[a][0] = coords[2 * (size_t)c.v[a]];
            c.x[a][1] = coords[2 * (size_t)c.v[a] + 1];
        }
        bal_cell_init(c, axi);
        double cW = 0.0;
        for (int q = 0; q < nq; ++q) {
            const double phi[3] = {1.0 - md->qp_x[q] - md->qp_y[q], md->qp_x[q], md->qp_y[q]};
            cW += md->qp_w[q] * c.detJ * two_pi * (c.rn[0] * phi[0] + c.rn[1] * phi[1] + c.rn[2] * phi[2]);
        }
        const double *ph = psi + (size_t)h * nvp;
        double gh[2], chk = 0.0;
        cur_grad(c.G, ph[c.v[0]], ph[c.v[1]], ph[c.v[2]], gh);
#pragma unroll
        for (int k = 0; k < CUR_MAX; ++k) {
            if (k > h) break;
            const double *pk = psi + (size_t)k * nvp;
            double gk[2];
            cur_grad(c.G, pk[c.v[0]], pk[c.v[1]], pk[c.v[2]], gk);
            const double t = cur_grad_dot(cW, gk, gh);
            acc[k] += t;
            chk += t;
        }
        bad |= !isfinite(chk);
    }
    cur_write_partials(acc, bad, sum_part, flag_part);
}

// ---- second pass -----------------------------------------------------------------------------------
// One workgroup: thread t brings the partials of workgroup t (nb of them, at most POST_BLOCKS = POST_THREADS), reduced
// slot by slot in the same fixed order.  The slots from n_slots on were not written by the first pass and are not read.
__global__ __launch_bounds__(POST_THREADS) void currents_finish_kernel(int nb, int n_slots,
                                                                      const double *__restrict__ sum_part,
                                                                      const int *__restrict__ flag_part,
                                                                      CurResult *__restrict__ res) {
    __shared__ double lds_sum[CUR_SUMS][POST_WAVES];
    const int t = threadIdx.x;
    double sv[CUR_SUMS];
#pragma unroll
    for (int k = 0; k < CUR_SUMS; ++k) sv[k] = (t < nb && k < n_slots) ? sum_part[(size_t)k * POST_BLOCKS + t] : 0.0;
    const int bad = t < nb && flag_part[t];
    const double s = block_sums(sv, lds_sum);
    const int any_bad = __syncthreads_or(bad);
    if (t < CUR_SUMS) res->sum[t] = s;
    if (t == 0) {
        res->not_finite = any_bad;
        res->pad_ = 0;
    }
}

// ---- the solve's vectors ---------------------------------------------------------------------------
// the free vertices' system: x = psi and b = rhs there, both 0 on the unit rows and the padding
__global__ void currents_split_kernel(int n, const unsigned char *__restrict__ fixed, const double *__restrict__ psi,
                                      const double *__restrict__ rhs, double *__restrict__ x, double *__restrict__ b) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool f = fixed[i] != 0;
    x[i] = f ? 0.0 : psi[i];
    b[i] = f ? 0.0 : rhs[i];
}

// the solved potential: the conductors' values as they were installed, the solution elsewhere
__global__ void currents_merge_kernel(int n, const unsigned char *__restrict__ fixed, const double *__restrict__ psi,
                                      const double *__restrict__ x, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = fixed[i] ? psi[i] : x[i];
}

// ---- host ------------------------------------------------------------------------------------------
void currents_release(Ctx &c) {
    Currents *k = c.currents;
    if (!k) return;
    k->cg.release();
    void *ptrs[] = {k->psi, k->sum_part, k->flag_part, k->result, k->psi_new, k->rhs, k->x, k->b, k->fixed};
    for (void *p : ptrs)
        if (p) hipFree(p);
    delete k;
    c.currents = nullptr;
}

namespace {

// the contexts the kernels are instantiated for (0), or the refusal
int cur_check_ctx(const Ctx &c, const char *who) {
    if (c.model_kind == 0 && !c.poisson)
        return refuse(who, "the model has no Poisson equation (the currents are those of its potential)");
    if (c.comm || c.n_owned != c.nv)
        return refuse(who, "the electrode currents run on one GPU (this context has a transport or ghost vertices)");
    if (c.model_kind == 1 && (c.neq < 3 || c.neq > 6))
        return refuse(who, std::to_string(c.neq) + " equations: 3 to 6 are built");
    return 0;
}

int cur_blocks(const Ctx &c) { return std::max(std::min((c.nc + POST_THREADS - 1) / POST_THREADS, POST_BLOCKS), 1); }

// the capacitance matrix of the potentials psi[n_psi][nvp] into cap: a launch and a read-back per column
int form_capacitance(Ctx &c, const double *psi, int n_psi, double cap[CUR_MAX][CUR_MAX]) {
    Currents &k = *c.currents;
    const int nb = cur_blocks(c);
    const dim3 t(POST_THREADS);
    for (int h = 0; h < n_psi; ++h) {
        if (c.model_kind == 0)
            hipLaunchKernelGGL((currents_capacitance_kernel<fedm_model_desc>), dim3(nb), t, 0, c.stream, c.nc, c.nvp,
                               c.d_model, c.d_coords, c.d_cells, psi, h, k.sum_part, k.flag_part);
        else
            hipLaunchKernelGGL((currents_capacitance_kernel<fedm_gd_desc>), dim3(nb), t, 0, c.stream, c.nc, c.nvp, c.d_gd,
                               c.d_coords, c.d_cells, psi, h, k.sum_part, k.flag_part);
        hipLaunchKernelGGL(currents_finish_kernel, dim3(1), t, 0, c.stream, nb, CUR_MAX, k.sum_part, k.flag_part, k.result);
        CurResult r;
        if (const int rc = read_result(c, r, c.currents->result)) return rc;
        for (int g = 0; g <= h; ++g) cap[g][h] = cap[h][g] = r.sum[g];
    }
    return 0;
}

int ensure_solve_buffers(Ctx &c) {
    Currents &k = *c.currents;
    if (k.fixed) return 0;
    const size_t nvp = (size_t)c.nvp;
    if (device_array<double>(k.psi_new, nullptr, nvp * CUR_MAX) || device_array<double>(k.rhs, nullptr, nvp * CUR_MAX) ||
        device_array<double>(k.x, nullptr, nvp) || device_array<double>(k.b, nullptr, nvp) ||
        device_array<unsigned char>(k.fixed, nullptr, nvp) || k.cg.alloc(nvp)) {
        // nothing half-made stays behind (the scratch has freed its own): the next call starts from nothing again
        void *ptrs[] = {k.psi_new, k.rhs, k.x, k.b, k.fixed};
        for (void *p : ptrs)
            if (p) hipFree(p);
        k.psi_new = k.rhs = k.x = k.b = nullptr;
        k.fixed = nullptr;
        return -1;
    }
    return 0;
}

}  // namespace

// (not in the unnamed namespace: fedm_circuit_measure runs the same pass and keeps its sums on the device)
void launch_currents(Ctx &c) {
    Currents &k = *c.currents;
    const int nb = cur_blocks(c);
    const dim3 t(POST_THREADS);
    if (c.model_kind == 0) {
        // (cur_check_ctx has required the Poisson equation: the PO switch is always true here)
        with_model_flags(c, [&](auto ns, auto, auto tab) {
            constexpr int NS = decltype(ns)::value;
            constexpr bool TAB = decltype(tab)::value;
            hipLaunchKernelGGL((currents_cell_kernel<NS, TAB>), dim3(nb), t, 0, c.stream, c.nc, c.nvp, c.d_model,
                               c.d_coords, c.d_cells, c.d_u, c.d_uold, c.d_uold1, c.dt, c.dt_old, k.psi, k.n_psi,
                               k.sum_part, k.flag_part);
        });
    } else {
        // (cur_check_ctx has refused the equation counts that are not built)
        with_gd_neq(c, [&](auto neq) {
            constexpr int NEQ = decltype(neq)::value;
            hipLaunchKernelGGL((gd_currents_cell_kernel<NEQ>), dim3(nb), t, 0, c.stream, c.nc, c.nv, c.nvp, c.d_gd,
                               c.d_gd_fields, c.d_coords, c.d_cells, c.d_u, c.d_uold, c.d_uold1, c.dt, c.dt_old, k.psi,
                               k.n_psi, k.sum_part, k.flag_part);
        });
    }
    hipLaunchKernelGGL(currents_finish_kernel, dim3(1), t, 0, c.stream, nb, CUR_SUMS, k.sum_part, k.flag_part, k.result);
}
}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_currents_setup(fedm_ctx *h, int n_psi, const double *psi) {
    const char *who = "fedm_currents_setup";
    if (!h || !psi) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (const int rc = cur_check_ctx(c, who)) return rc;
    if (n_psi < 1 || n_psi > CUR_MAX)
        return refuse(who, std::to_string(n_psi) + " weighting potentials, 1 to " + std::to_string(CUR_MAX) + " are possible");
    for (size_t i = 0; i < (size_t)n_psi * c.nv; ++i)
        if (!std::isfinite(psi[i]))
            return refuse(who, "psi[" + std::to_string(i / c.nv) + "][" + std::to_string(i % c.nv) + "] is not finite");
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (!c.currents) {
        Currents *k = new Currents();
        c.currents = k;
        if (device_array<double>(k->psi, nullptr, (size_t)c.nvp * CUR_MAX) ||
            device_array<double>(k->sum_part, nullptr, (size_t)CUR_SUMS * POST_BLOCKS) ||
            device_array<int>(k->flag_part, nullptr, POST_BLOCKS) || device_array<CurResult>(k->result, nullptr, 1)) {
            currents_release(c);
            return -1;
        }
    }
    Currents &k = *c.currents;
    k.n_psi = 0;   // (until the capacitance stands: a failure on the way leaves no half set-up)
    FEDM_HIP_CHECK(hipMemset(k.psi, 0, sizeof(double) * c.nvp * CUR_MAX));
    for (int g = 0; g < n_psi; ++g)
        FEDM_HIP_CHECK(hipMemcpy(k.psi + (size_t)g * c.nvp, psi + (size_t)g * c.nv, sizeof(double) * c.nv, hipMemcpyHostToDevice));
    for (auto &row : k.cap)
        for (double &v : row) v = 0.0;
    if (const int rc = form_capacitance(c, k.psi, n_psi, k.cap)) return rc;
    k.n_psi = n_psi;
    return 0;
}

int fedm_currents_solve(fedm_ctx *h, const fedm_photo_hierarchy *laplace, const double *rhs, double rtol, int max_it,
                        int iterations[FEDM_CURRENTS_MAX]) {
    const char *who = "fedm_currents_solve";
    if (!h || !laplace || !rhs) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (const int rc = cur_check_ctx(c, who)) return rc;
    if (!c.currents || c.currents->n_psi == 0) return refuse(who, "fedm_currents_setup has not been called");
    Currents &k = *c.currents;
    if (!(rtol > 0.0) || max_it < 0) return refuse(who, "rtol must be positive and max_it not negative");
    for (size_t i = 0; i < (size_t)k.n_psi * c.nv; ++i)
        if (!std::isfinite(rhs[i]))
            return refuse(who, "rhs[" + std::to_string(i / c.nv) + "][" + std::to_string(i % c.nv) + "] is not finite");
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (ensure_solve_buffers(c)) return -1;
    EllMat A;
    Amg *M = nullptr;
    auto drop = [&] { release_hierarchy(A, M); };
    if (const int rc = upload_hierarchy(c, who, "", *laplace, A, M)) {
        drop();
        return rc;
    }
    // the conductors' vertices: the unit rows of the eliminated operator (and the padding)
    const fedm_csr &A0 = laplace->A[0];
    std::vector<unsigned char> fixed((size_t)c.nvp, 1);
    for (int v = 0; v < c.nv; ++v) {
        bool unit = true;
        for (int64_t j = A0.indptr[v]; j < A0.indptr[v + 1] && unit; ++j)
            unit = A0.values[j] == (A0.indices[j] == v ? 1.0 : 0.0);
        fixed[v] = unit && A0.indptr[v + 1] > A0.indptr[v] ? 1 : 0;
    }
    const size_t nvp = (size_t)c.nvp;
    // (between A / M and drop(): an early return would leak them, so the uploads' status is collected and looked at once)
    hipError_t up = hipMemcpy(k.fixed, fixed.data(), nvp, hipMemcpyHostToDevice);
    if (up == hipSuccess) up = hipMemset(k.rhs, 0, sizeof(double) * nvp * CUR_MAX);
    for (int g = 0; g < k.n_psi && up == hipSuccess; ++g)
        up = hipMemcpy(k.rhs + g * nvp, rhs + (size_t)g * c.nv, sizeof(double) * c.nv, hipMemcpyHostToDevice);
    if (up == hipSuccess) up = hipMemsetAsync(k.psi_new, 0, sizeof(double) * nvp * CUR_MAX, c.stream);
    if (up != hipSuccess) {
        drop();
        FEDM_HIP_CHECK(up);
    }
    const dim3 gv((c.nvp + 255) / 256), bl(256);
    int rc = 0;
    for (int g = 0; g < CUR_MAX; ++g) {
        int its = 0;
        if (g < k.n_psi && rc == 0) {
            hipLaunchKernelGGL(currents_split_kernel, gv, bl, 0, c.stream, c.nvp, k.fixed, k.psi + g * nvp, k.rhs + g * nvp,
                               k.x, k.b);
            const ScalarCgResult cg = scalar_pcg(c, k.cg, A, M, k.b, k.x, rtol, max_it);
            its = cg.it;
            rc = cg.status(rtol);
            hipLaunchKernelGGL(currents_merge_kernel, gv, bl, 0, c.stream, c.nvp, k.fixed, k.psi + g * nvp, k.x,
                               k.psi_new + g * nvp);
        }
        if (iterations) iterations[g] = its;
    }
    double cap[CUR_MAX][CUR_MAX] = {};
    if (rc == 0) {
        if (const int rc2 = form_capacitance(c, k.psi_new, k.n_psi, cap)) {
            drop();
            return rc2;
        }
        // every potential converged: the candidates become the installed ones
        std::swap(k.psi, k.psi_new);
        for (int g = 0; g < CUR_MAX; ++g)
            for (int j = 0; j < CUR_MAX; ++j) k.cap[g][j] = cap[g][j];
    }
    const hipError_t e = hipStreamSynchronize(c.stream);
    drop();
    FEDM_HIP_CHECK(e);
    FEDM_HIP_CHECK(hipGetLastError());
    return rc;
}

int fedm_currents_get_psi(fedm_ctx *h, double *psi) {
    const char *who = "fedm_currents_get_psi";
    if (!h || !psi) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (!c.currents || c.currents->n_psi == 0) return refuse(who, "fedm_currents_setup has not been called");
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    for (int g = 0; g < c.currents->n_psi; ++g)
        FEDM_HIP_CHECK(hipMemcpy(psi + (size_t)g * c.nv, c.currents->psi + (size_t)g * c.nvp, sizeof(double) * c.nv,
                                 hipMemcpyDeviceToHost));
    return 0;
}

int fedm_currents(fedm_ctx *h, struct fedm_currents *out) {
    const char *who = "fedm_currents";
    if (!h || !out) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (const int rc = cur_check_ctx(c, who)) return rc;
    if (!c.currents || c.currents->n_psi == 0) return refuse(who, "fedm_currents_setup has not been called");
    const Currents &k = *c.currents;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    launch_currents(c);
    CurResult r;
    if (const int rc = read_result(c, r, c.currents->result)) return rc;
    *out = {};
    for (int g = 0; g < k.n_psi; ++g) {
        out->conduction[g] = r.sum[CUR_COND + g];
        out->displacement[g] = r.sum[CUR_DISP + g];
        out->coupling[g] = r.sum[CUR_COUP + g];
        out->induced_charge[g] = r.sum[CUR_CHARGE + g];
        for (int j = 0; j < k.n_psi; ++j) out->capacitance[g][j] = k.cap[g][j];
    }
    out->n_psi = k.n_psi;
    out->finite = r.not_finite ? 0 : 1;
    return 0;
}

}  // extern "C"
