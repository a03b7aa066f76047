// External circuit of the driven electrodes (include/fedm_hip.h, fedm_circuit_setup / fedm_circuit_measure /
// fedm_circuit_advance / fedm_circuit_get): a source, a series resistance and a stray capacitance per conductor of the
// electrode currents' set-up, closed on the device.  The measure runs currents.hip's cell pass for the conduction (its
// sums stay in Currents::result) and a pass of its own for the conductance -- the plasma seen from the electrodes at
// frozen densities and coefficients -- in the pattern of the post-processing passes: a thread per cell writes
// slot-major partials, one workgroup reduces them in a fixed order, no floating-point atomics.  The advance is one
// thread's algebra on an 8 x 8 system at the most; the apply writes the conductors' potentials into the Dirichlet
// values the Newton solve reads.  Nothing is read back between the three unless the caller asks for the record.
// A cell's part of G does not depend on the pair: S = sum_s Z_s^2 mu_s sum W n_s, then S grad psi_g . grad psi_h for
// g <= h, at most 36 sums in compile-time slots (cur_accumulate's way).
#include "circuit.hpp"

#include <cmath>
#include <cstring>
#include <vector>

#include "element.hpp"
#include "gd_balance.hpp"
#include "postproc.hpp"
#include "solver.hpp"

namespace fedm {

// S grad psi_g . grad psi_h of one cell into the slots of the pairs g <= h < n_psi; returns their sum for the
// not-finite flag
__device__ __forceinline__ double circ_accumulate(double (&acc)[CIRC_SLOTS], double S, const double G[3][2],
                                                  const int v[3], const double *__restrict__ psi, int nvp, int n_psi) {
    double gp[CUR_MAX][2];
#pragma unroll
    for (int k = 0; k < CUR_MAX; ++k) {
        gp[k][0] = gp[k][1] = 0.0;
        if (k >= n_psi) continue;
        const double *pk = psi + (size_t)k * nvp;
        cur_grad(G, pk[v[0]], pk[v[1]], pk[v[2]], gp[k]);
    }
    double chk = 0.0;
#pragma unroll
    for (int g = 0; g < CUR_MAX; ++g) {
#pragma unroll
        for (int h = g; h < CUR_MAX; ++h) {
            if (h >= n_psi) continue;
            const double t = cur_grad_dot(S, gp[g], gp[h]);
            acc[circ_slot(g, h)] += t;
            chk += t;
        }
    }
    return chk;
}

// ---- the cells, LFA ----------------------------------------------------------------------------------
// |E|, the mobilities and the densities' sums as currents_cell_kernel has them
template <int NS, bool TAB>
__global__ __launch_bounds__(POST_THREADS) void circuit_conductance_kernel(
    int nc, int nvp, const fedm_model_desc *__restrict__ md, const double *__restrict__ coords,
    const int *__restrict__ cells, const double *__restrict__ u, const double *__restrict__ psi, int n_psi,
    double *__restrict__ sum_part, int *__restrict__ flag_part) {
    constexpr int NEQ = NS + 1, IPHI = NS;
    const double two_pi = 6.283185307179586476925286766559;
    const bool axi = md->axisymmetric != 0, lin = md->linear_representation != 0;
    const int nq = md->n_qp;
    double acc[CIRC_SLOTS];
#pragma unroll
    for (int k = 0; k < CIRC_SLOTS; ++k) acc[k] = 0.0;
    bool bad = false;
    for (int cell = blockIdx.x * blockDim.x + threadIdx.x; cell < nc; cell += gridDim.x * blockDim.x) {
        int v[3];
        double x[3][2], U[3][NEQ];
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
        }
        CellGeom cg;
        cg.init(x, axi);
        double gP[2];
        cur_grad(cg.G, U[0][IPHI], U[1][IPHI], U[2][IPHI], gP);
        const double Em = sqrt(gP[0] * gP[0] + gP[1] * gP[1]), invEm = 1.0 / Em, lnE = log(Em);
        double cN[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) cN[s] = 0.0;
        for (int q = 0; q < nq; ++q) {
            const double xq = md->qp_x[q], yq = md->qp_y[q];
            const double phi[3] = {1.0 - xq - yq, xq, yq};
            const double rq = cg.rn[0] * phi[0] + cg.rn[1] * phi[1] + cg.rn[2] * phi[2];
            const double W = md->qp_w[q] * cg.detJ * two_pi * rq;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double us = U[0][s] * phi[0] + U[1][s] * phi[1] + U[2][s] * phi[2];
                cN[s] += W * (lin ? us : exp(us));
            }
        }
        double S = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (md->eq_type[s] != FEDM_EQ_DRIFT_DIFFUSION_REACTION || md->has_drift_w[s]) continue;
            double muv, mud;
            termsum_eval<TAB>(md, md->mu[s], Em, invEm, lnE, muv, mud);
            S += (md->Z[s] * md->Z[s]) * muv * cN[s];
        }
        const double chk = circ_accumulate(acc, S, cg.G, v, psi, nvp, n_psi);
        bad |= !isfinite(chk + S);
    }
    cur_write_partials(acc, bad, sum_part, flag_part);
}

// ---- the cells, LMEA ---------------------------------------------------------------------------------
// The semi-implicit mobilities and the densities at every quadrature point as bal_point gives them; the species whose
// flux gd_currents_cell_kernel takes with a drift part: the electrons and the 'drift-diffusion-reaction' ones
template <int NEQ>
__global__ __launch_bounds__(POST_THREADS) void gd_circuit_conductance_kernel(
    int nc, int nv, int nvp, const fedm_gd_desc *__restrict__ md, const double *__restrict__ fields,
    const double *__restrict__ coords, const int *__restrict__ cells, const double *__restrict__ u,
    const double *__restrict__ psi, int n_psi, double *__restrict__ sum_part, int *__restrict__ flag_part) {
    constexpr int ns = NEQ - 1, ie = ns - 1;
    const double two_pi = 6.283185307179586476925286766559;
    const int nr = md->n_reactions, nq = md->n_qp;
    double acc[CIRC_SLOTS];
#pragma unroll
    for (int k = 0; k < CIRC_SLOTS; ++k) acc[k] = 0.0;
    bool bad = false;
    for (int cell = blockIdx.x * blockDim.x + threadIdx.x; cell < nc; cell += gridDim.x * blockDim.x) {
        BalCell c;
        double U[3][NEQ];
        bad |= bal_load_cell<NEQ>(cell, md, coords, cells, u, c, U);
        double S = 0.0;
        for (int q = 0; q < nq; ++q) {
            const double phi[3] = {1.0 - md->qp_x[q] - md->qp_y[q], md->qp_x[q], md->qp_y[q]};
            const double rq = c.rn[0] * phi[0] + c.rn[1] * phi[1] + c.rn[2] * phi[2];
            const double W = md->qp_w[q] * c.detJ * two_pi * rq;
            BalPoint<NEQ> p;
            bal_point<NEQ>(fields, nv, nr, c, U, phi, p);
            double sp = 0.0;
#pragma unroll
            for (int s = 1; s < ns; ++s) {
                if (s != ie && md->eq_type[s] != FEDM_EQ_DRIFT_DIFFUSION_REACTION) continue;
                sp += (md->sign[s] * md->sign[s]) * (p.mu[s] * p.e[s]);
            }
            S += W * sp;
        }
        const double chk = circ_accumulate(acc, S, c.G, c.v, psi, nvp, n_psi);
        bad |= !isfinite(chk + S);
    }
    cur_write_partials(acc, bad, sum_part, flag_part);
}

// ---- the measure's finish ----------------------------------------------------------------------------
// One workgroup: thread t brings the partials of workgroup t, reduced slot by slot in the fixed order; [g][h] and
// [h][g] from the one sum.  Thread 0 moves the history (U_old1 <- U_old <- U) and takes the conduction and the flag
// that currents_finish_kernel has left on the device.
__global__ __launch_bounds__(POST_THREADS) void circuit_finish_kernel(int nb, int n, const double *__restrict__ sum_part,
                                                                     const int *__restrict__ flag_part,
                                                                     const CurResult *__restrict__ cur,
                                                                     CircState *__restrict__ st) {
    __shared__ double lds_sum[CIRC_SLOTS][POST_WAVES];
    const int t = threadIdx.x;
    double sv[CIRC_SLOTS];
#pragma unroll
    for (int k = 0; k < CIRC_SLOTS; ++k) sv[k] = t < nb ? sum_part[(size_t)k * POST_BLOCKS + t] : 0.0;
    const int bad = t < nb && flag_part[t];
    const double s = block_sums(sv, lds_sum);
    const int any_bad = __syncthreads_or(bad);
    if (t < CIRC_SLOTS) {
        int g = 0, first = 0;   // the pair of slot t
        while (t >= first + (CUR_MAX - g)) {
            first += CUR_MAX - g;
            ++g;
        }
        const int h = g + (t - first);
        const double val = h < n ? s : 0.0;
        st->G[g][h] = val;
        st->G[h][g] = val;
    }
    if (t == 0) {
        for (int g = 0; g < CUR_MAX; ++g) {
            st->Uo1[g] = st->Uo[g];
            st->Uo[g] = st->U[g];
            st->cond[g] = g < n ? cur->sum[CUR_COND + g] : 0.0;
        }
        st->measure_bad = (any_bad || cur->not_finite) ? 1 : 0;
        st->flag = st->measure_bad ? CIRC_FLAG_MEASURE : 0;
    }
}

// ---- the advance -------------------------------------------------------------------------------------
// One workgroup, thread 0: the driven electrodes' system (the header has it), Gaussian elimination with partial
// pivoting in plain doubles.  U is written only when every value is finite.
__global__ void circuit_advance_kernel(CircStep p, CircState *__restrict__ st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double e = FEDM_ELEMENTARY_CHARGE, eps0 = FEDM_VACUUM_PERMITTIVITY;
    const int n = p.n;
    const double w = p.dt / p.dt_old, wp1 = 1.0 + w;
    const double a = (1.0 + 2.0 * w) / (wp1 * p.dt);
    double hist[CUR_MAX], Un[CUR_MAX];
    int drv[CUR_MAX], nd = 0;
    for (int g = 0; g < n; ++g) {
        hist[g] = (-(wp1 * wp1) * st->Uo[g] + (w * w) * st->Uo1[g]) / (wp1 * p.dt);
        Un[g] = p.V[g];   // the ideal ones; the driven ones are overwritten below
        if (p.R[g] > 0.0) drv[nd++] = g;
    }
    int flag = st->measure_bad ? CIRC_FLAG_MEASURE : 0;
    double A[CUR_MAX][CUR_MAX + 1];
    for (int i = 0; i < nd; ++i) {
        const int g = drv[i];
        double b = p.V[g] / p.R[g] - e * st->cond[g] - p.Cp[g] * hist[g];
        for (int h = 0; h < n; ++h) {
            b += e * st->G[g][h] * st->Uo[h] - eps0 * st->C[g][h] * hist[h];
            if (!(p.R[h] > 0.0)) b -= (a * eps0 * st->C[g][h] + e * st->G[g][h]) * p.V[h];
        }
        for (int j = 0; j < nd; ++j) {
            const int h = drv[j];
            A[i][j] = a * eps0 * st->C[g][h] + e * st->G[g][h] + (i == j ? 1.0 / p.R[g] + a * p.Cp[g] : 0.0);
        }
        A[i][nd] = b;
    }
    for (int k = 0; k < nd && !(flag & CIRC_FLAG_SINGULAR); ++k) {
        int piv = k;
        for (int i = k + 1; i < nd; ++i)
            if (fabs(A[i][k]) > fabs(A[piv][k])) piv = i;
        if (!(fabs(A[piv][k]) > 0.0) || !isfinite(A[piv][k])) {
            flag |= CIRC_FLAG_SINGULAR;
            break;
        }
        if (piv != k)
            for (int j = k; j <= nd; ++j) {
                const double tmp = A[k][j];
                A[k][j] = A[piv][j];
                A[piv][j] = tmp;
            }
        for (int i = k + 1; i < nd; ++i) {
            const double f = A[i][k] / A[k][k];
            for (int j = k; j <= nd; ++j) A[i][j] -= f * A[k][j];
        }
    }
    if (!(flag & CIRC_FLAG_SINGULAR)) {
        for (int i = nd - 1; i >= 0; --i) {
            double s = A[i][nd];
            for (int j = i + 1; j < nd; ++j) s -= A[i][j] * Un[drv[j]];
            Un[drv[i]] = s / A[i][i];
        }
    }
    double dU[CUR_MAX], lead[CUR_MAX], chk = 0.0;
    for (int g = 0; g < n; ++g) {
        dU[g] = a * Un[g] + hist[g];
        chk += Un[g] + dU[g];
    }
    for (int g = 0; g < n; ++g) {
        if (p.R[g] > 0.0) {
            lead[g] = (p.V[g] - Un[g]) / p.R[g];
        } else {
            double I = e * st->cond[g] + p.Cp[g] * dU[g];
            for (int h = 0; h < n; ++h) I += e * st->G[g][h] * (Un[h] - st->Uo[h]) + eps0 * st->C[g][h] * dU[h];
            lead[g] = I;
        }
        chk += lead[g];
    }
    if (!flag && !isfinite(chk)) flag |= CIRC_FLAG_RESULT;
    if (!flag)
        for (int g = 0; g < n; ++g) {
            st->U[g] = Un[g];
            st->dUdt[g] = dU[g];
            st->lead[g] = lead[g];
        }
    st->flag = flag;
}

// ---- the apply ---------------------------------------------------------------------------------------
// A thread per Dirichlet entry (the context's order); entries of no electrode are not written
__global__ void circuit_apply_kernel(int n_dir, const int8_t *__restrict__ entry, const CircState *__restrict__ st,
                                     double *__restrict__ dir_vals) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_dir) return;
    const int g = entry[k];
    if (g >= 0) dir_vals[k] = st->U[g];
}

// ---- host ------------------------------------------------------------------------------------------
void circuit_release(Ctx &c) {
    Circuit *k = c.circuit;
    if (!k) return;
    void *ptrs[] = {k->state, k->entry, k->sum_part, k->flag_part};
    for (void *p : ptrs)
        if (p) hipFree(p);
    delete k;
    c.circuit = nullptr;
}

namespace {

int circ_check_ctx(const Ctx &c, const char *who) {
    if (c.model_kind == 0 && !c.poisson)
        return refuse(who, "the model has no Poisson equation (the electrodes are conductors of its potential)");
    if (c.comm || c.n_owned != c.nv)
        return refuse(who, "the external circuit runs on one GPU (this context has a transport or ghost vertices)");
    return 0;
}

void fill_state(const CircState &s, int n, struct fedm_circuit_state *out) {
    *out = {};
    for (int g = 0; g < n; ++g) {
        out->U[g] = s.U[g];
        out->U_old[g] = s.Uo[g];
        out->U_old1[g] = s.Uo1[g];
        out->dUdt[g] = s.dUdt[g];
        out->lead_current[g] = s.lead[g];
        out->conduction[g] = s.cond[g];
        for (int h = 0; h < n; ++h) out->conductance[g][h] = s.G[g][h];
    }
    out->n = n;
    out->flag = s.flag;
}

}  // namespace
}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_circuit_setup(fedm_ctx *h, const fedm_circuit_desc *d) {
    const char *who = "fedm_circuit_setup";
    if (!h || !d) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (const int rc = circ_check_ctx(c, who)) return rc;
    if (!c.currents || c.currents->n_psi == 0) return refuse(who, "fedm_currents_setup has not been called");
    if (d->n != c.currents->n_psi)
        return refuse(who, std::to_string(d->n) + " electrodes, the currents set-up has " + std::to_string(c.currents->n_psi));
    for (int g = 0; g < d->n; ++g) {
        if (!std::isfinite(d->R[g]) || d->R[g] < 0.0) return refuse(who, "R[" + std::to_string(g) + "] is negative or not finite");
        if (!std::isfinite(d->Cp[g]) || d->Cp[g] < 0.0) return refuse(who, "Cp[" + std::to_string(g) + "] is negative or not finite");
        if (!std::isfinite(d->U0[g])) return refuse(who, "U0[" + std::to_string(g) + "] is not finite");
    }
    if (c.n_dir > 0 && !d->electrode_of_entry) return refuse(who, "null argument (electrode_of_entry)");
    for (int k = 0; k < c.n_dir; ++k)
        if (d->electrode_of_entry[k] < -1 || d->electrode_of_entry[k] >= d->n)
            return refuse(who, "electrode_of_entry[" + std::to_string(k) + "] = " + std::to_string((int)d->electrode_of_entry[k]) +
                                   " outside -1.." + std::to_string(d->n - 1));
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (!c.circuit) {
        Circuit *k = new Circuit();
        c.circuit = k;
        if (device_array<CircState>(k->state, nullptr, 1) || device_array<int8_t>(k->entry, nullptr, (size_t)c.n_dir) ||
            device_array<double>(k->sum_part, nullptr, (size_t)CIRC_SLOTS * POST_BLOCKS) ||
            device_array<int>(k->flag_part, nullptr, POST_BLOCKS)) {
            circuit_release(c);
            return -1;
        }
    }
    Circuit &k = *c.circuit;
    k.n = 0;   // (until everything stands: a failure on the way leaves no half set-up)
    k.measured = false;
    std::vector<int8_t> entry((size_t)c.n_dir);
    for (int i = 0; i < c.n_dir; ++i) entry[i] = d->electrode_of_entry[c.dir_perm[i]];   // the context's order
    if (c.n_dir) FEDM_HIP_CHECK(hipMemcpy(k.entry, entry.data(), (size_t)c.n_dir, hipMemcpyHostToDevice));
    CircState s = {};
    for (int g = 0; g < d->n; ++g) {
        s.U[g] = s.Uo[g] = s.Uo1[g] = d->U0[g];
        k.R[g] = d->R[g];
        k.Cp[g] = d->Cp[g];
    }
    std::memcpy(k.cap, c.currents->cap, sizeof(k.cap));
    std::memcpy(s.C, k.cap, sizeof(k.cap));
    FEDM_HIP_CHECK(hipMemcpy(k.state, &s, sizeof(s), hipMemcpyHostToDevice));
    k.n = d->n;
    return 0;
}

int fedm_circuit_measure(fedm_ctx *h) {
    const char *who = "fedm_circuit_measure";
    if (!h) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (!c.circuit || c.circuit->n == 0) return refuse(who, "fedm_circuit_setup has not been called");
    Circuit &k = *c.circuit;
    if (!c.currents || c.currents->n_psi != k.n)
        return refuse(who, "the currents set-up has changed its number of potentials since fedm_circuit_setup");
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (std::memcmp(k.cap, c.currents->cap, sizeof(k.cap)) != 0) {   // the potentials were solved for again
        std::memcpy(k.cap, c.currents->cap, sizeof(k.cap));
        FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
        FEDM_HIP_CHECK(hipMemcpy(&k.state->C, k.cap, sizeof(k.cap), hipMemcpyHostToDevice));
    }
    launch_currents(c);
    const int nb = std::max(std::min((c.nc + POST_THREADS - 1) / POST_THREADS, POST_BLOCKS), 1);
    const dim3 t(POST_THREADS);
    const double *psi = c.currents->psi;
    if (c.model_kind == 0) {
        with_model_flags(c, [&](auto ns, auto, auto tab) {
            constexpr int NS = decltype(ns)::value;
            constexpr bool TAB = decltype(tab)::value;
            hipLaunchKernelGGL((circuit_conductance_kernel<NS, TAB>), dim3(nb), t, 0, c.stream, c.nc, c.nvp, c.d_model,
                               c.d_coords, c.d_cells, c.d_u, psi, k.n, k.sum_part, k.flag_part);
        });
    } else {
        with_gd_neq(c, [&](auto neq) {
            constexpr int NEQ = decltype(neq)::value;
            hipLaunchKernelGGL((gd_circuit_conductance_kernel<NEQ>), dim3(nb), t, 0, c.stream, c.nc, c.nv, c.nvp, c.d_gd,
                               c.d_gd_fields, c.d_coords, c.d_cells, c.d_u, psi, k.n, k.sum_part, k.flag_part);
        });
    }
    hipLaunchKernelGGL(circuit_finish_kernel, dim3(1), t, 0, c.stream, nb, k.n, k.sum_part, k.flag_part, c.currents->result,
                       k.state);
    FEDM_HIP_CHECK(hipGetLastError());
    k.measured = true;
    return 0;
}

int fedm_circuit_advance(fedm_ctx *h, const double V[FEDM_CURRENTS_MAX], struct fedm_circuit_state *out) {
    const char *who = "fedm_circuit_advance";
    if (!h || !V) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (!c.circuit || c.circuit->n == 0) return refuse(who, "fedm_circuit_setup has not been called");
    Circuit &k = *c.circuit;
    if (!k.measured) return refuse(who, "fedm_circuit_measure has not been called since the set-up");
    CircStep p = {};
    p.dt = c.dt;
    p.dt_old = c.dt_old;
    p.n = k.n;
    for (int g = 0; g < k.n; ++g) {
        p.V[g] = V[g];
        p.R[g] = k.R[g];
        p.Cp[g] = k.Cp[g];
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    hipLaunchKernelGGL(circuit_advance_kernel, dim3(1), dim3(64), 0, c.stream, p, k.state);
    if (c.n_dir > 0)
        hipLaunchKernelGGL(circuit_apply_kernel, dim3((c.n_dir + 255) / 256), dim3(256), 0, c.stream, c.n_dir, k.entry,
                           k.state, c.d_dir_vals);
    FEDM_HIP_CHECK(hipGetLastError());
    if (out) {
        CircState s;
        if (const int rc = read_result(c, s, k.state)) return rc;
        fill_state(s, k.n, out);
    }
    return 0;
}

int fedm_circuit_get(fedm_ctx *h, struct fedm_circuit_state *out) {
    const char *who = "fedm_circuit_get";
    if (!h || !out) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (!c.circuit || c.circuit->n == 0) return refuse(who, "fedm_circuit_setup has not been called");
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    CircState s;
    if (const int rc = read_result(c, s, c.circuit->state)) return rc;
    fill_state(s, c.circuit->n, out);
    return 0;
}

}  // extern "C"
