// Field output (include/fedm_hip.h, fedm_fields_setup / fedm_probe_setup / fedm_fields): derived nodal fields and point
// probes from the resident state.  Per state one pass over the cells for ALL projected requests of the call (a thread
// per cell stores its three corner entries per request) and one over the vertices (a thread per (vertex, request):
// pointwise kinds from the state, projected kinds by adding the vertex's entries in the ascending (cell, corner) order of
// the list -- photo.hip's store-then-sum load vector), the blend of two states, the probes, and one read-back.  Plain
// launches on the context's stream; no kernel caps its grid, none waits for another workgroup, and nothing adds with
// floating-point atomics: a call is bitwise reproducible.  The set-up, the consistent solve, the blend, the probes and
// the read-back serve the LMEA family's fedm_gd_fields as well (gd_fields.hip has its cell and vertex pass): fields.hpp
// declares what the two share; the host's helpers are postproc.hpp's.
#include "fields.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "comm.hpp"
#include "element.hpp"
#include "postproc.hpp"
#include "solver.hpp"

namespace fedm {

// the projected requests of a call: slot k of cell_b belongs to request req[k] of the call
struct FieldCellReqs {
    int n;
    int kind[FEDM_FIELDS_MAX_REQ], index[FEDM_FIELDS_MAX_REQ];
};
// every request of a call: slot[k] >= 0: its slot of cell_b (projected), -1: pointwise
struct FieldVertexReqs {
    int n;
    int kind[FEDM_FIELDS_MAX_REQ], index[FEDM_FIELDS_MAX_REQ], slot[FEDM_FIELDS_MAX_REQ];
};

// ---- the cells -------------------------------------------------------------------------------------
// A thread per cell.  grad(Phi), |E| and the coefficients once per cell as Element::setup has them; a request's
// integrand at the model's quadrature points is  f(x_q) = A + B g(x_q)  with cell constants A, B and g the density (or,
// linear representation, the unknown) of one species, or a reaction's product of densities; the plain measure
// W_q = qp_w[q] |det J|.  The state is read where it is needed (run-time species and reaction indices address memory,
// never registers).
template <int NS, bool PO, bool TAB>
__global__ __launch_bounds__(FIELDS_THREADS) void fields_cell_kernel(int nc, const fedm_model_desc *__restrict__ md,
                                                                     const double *__restrict__ coords,
                                                                     const int *__restrict__ cells,
                                                                     const double *__restrict__ u, FieldCellReqs rq,
                                                                     double *__restrict__ cell_b) {
    constexpr int NEQ = NS + (PO ? 1 : 0);
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= nc) return;
    int v[3];
    double x[3][2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v[a] = cells[3 * (size_t)cell + a];
        x[a][0] = coords[2 * (size_t)v[a]];
        x[a][1] = coords[2 * (size_t)v[a] + 1];
    }
    const bool lin = md->linear_representation != 0;
    CellGeom cg;
    cg.init(x, md->axisymmetric);
    double gP[2] = {0.0, 0.0}, Em = 1.0, invEm = 1.0;
    if (PO) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double pa = u[(size_t)v[a] * NEQ + NEQ - 1];
            gP[0] += pa * cg.G[a][0];
            gP[1] += pa * cg.G[a][1];
        }
        Em = sqrt(gP[0] * gP[0] + gP[1] * gP[1]);
        invEm = 1.0 / Em;
    }
    const double lnE = log(Em);
    const int nq = md->n_qp;
    for (int k = 0; k < rq.n; ++k) {
        const int kind = rq.kind[k], idx = rq.index[k];
        double A = 0.0, B = 0.0, ua[3] = {0.0, 0.0, 0.0};
        int g_of = 0;   // 0: f = A, 1: g = n_idx (linear representation: u_idx), 2: g = prod_i n_i^power[idx][i]
        if (kind == FEDM_FIELD_E_R) {
            A = -gP[0];
        } else if (kind == FEDM_FIELD_E_Z) {
            A = -gP[1];
        } else if (kind == FEDM_FIELD_E_NORM) {
            A = Em;
        } else if (kind == FEDM_FIELD_RATE) {
            double kd;
            termsum_eval<TAB>(md, md->k[idx], Em, invEm, lnE, B, kd);
            g_of = 2;
        } else {   // FLUX_R, FLUX_Z
            const int d = kind == FEDM_FIELD_FLUX_Z ? 1 : 0;
            const int et = md->eq_type[idx];
            if (et != FEDM_EQ_REACTION) {
                double Dv, Dd, gu = 0.0, w = 0.0;
                termsum_eval<TAB>(md, md->D[idx], Em, invEm, lnE, Dv, Dd);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    ua[a] = u[(size_t)v[a] * NEQ + idx];
                    gu += ua[a] * cg.G[a][d];
                }
                if (et == FEDM_EQ_DRIFT_DIFFUSION_REACTION) {
                    if (md->has_drift_w[idx]) {
                        w = md->drift_w[idx][d];
                    } else if (PO) {
                        double muv, mud;
                        termsum_eval<TAB>(md, md->mu[idx], Em, invEm, lnE, muv, mud);
                        w = -md->Z[idx] * muv * gP[d];
                    }
                }
                // logarithmic: n (-D grad u + w); linear: -D grad u + w u
                if (lin) {
                    A = -Dv * gu;
                    B = w;
                } else {
                    B = -Dv * gu + w;
                }
                g_of = 1;
            }
        }
        double acc[3] = {0.0, 0.0, 0.0};
        for (int q = 0; q < nq; ++q) {
            const double xq = md->qp_x[q], yq = md->qp_y[q];
            const double phi[3] = {1.0 - xq - yq, xq, yq};
            const double W = md->qp_w[q] * cg.detJ;
            double f = A;
            if (g_of == 1) {
                const double us = ua[0] * phi[0] + ua[1] * phi[1] + ua[2] * phi[2];
                f = A + B * (lin ? us : exp(us));
            } else if (g_of == 2) {
                double prod = 1.0;
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const int P = md->power[idx][i];
                    if (!P) continue;
                    const double ui = u[(size_t)v[0] * NEQ + i] * phi[0] + u[(size_t)v[1] * NEQ + i] * phi[1] +
                                      u[(size_t)v[2] * NEQ + i] * phi[2];
                    const double n = lin ? ui : exp(ui);
                    for (int e = 0; e < P; ++e) prod *= n;
                }
                f = B * prod;
            }
            const double Wf = W * f;
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[a] += Wf * phi[a];
        }
        double *dst = cell_b + ((size_t)k * nc + cell) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) dst[a] = acc[a];
    }
}

// ---- the vertices ----------------------------------------------------------------------------------
// A thread per (vertex, request), blockIdx.y the request.  Pointwise kinds from the state; projected kinds: the vertex's
// entries in the order of the list, divided by the lumped mass (rhs_of < 0) or, for the one request rhs_of, left as the
// right-hand side of the consistent solve.  Ghost vertices and the padding get 0.  Request 0's threads look at every
// component of the owned vertices' state for the flag; every result is looked at as well.
__global__ __launch_bounds__(FIELDS_THREADS) void fields_vertex_kernel(
    int n_owned, int nvp, int nc, int ns, int neq, const fedm_model_desc *__restrict__ md, const double *__restrict__ u,
    const int *__restrict__ v_ptr, const int *__restrict__ v_idx, const double *__restrict__ m,
    const double *__restrict__ cell_b, FieldVertexReqs rq, int raw_sums, double *__restrict__ dst, int *__restrict__ flag) {
#pragma clang fp contract(off)
    const int v = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (v >= nvp) return;
    double val = 0.0;
    bool bad = false;
    if (v < n_owned) {
        const int kind = rq.kind[k], idx = rq.index[k], slot = rq.slot[k];
        const bool lin = md->linear_representation != 0;
        if (k == 0)
            for (int e = 0; e < neq; ++e) bad |= !isfinite(u[(size_t)v * neq + e]);
        if (slot >= 0) {
            const double *b = cell_b + (size_t)slot * nc * 3;
            double s = 0.0;
            for (int j = v_ptr[v]; j < v_ptr[v + 1]; ++j) s += b[v_idx[j]];
            val = raw_sums ? s : s / m[v];
        } else if (kind == FEDM_FIELD_STATE) {
            val = u[(size_t)v * neq + idx];
        } else if (kind == FEDM_FIELD_DENSITY) {
            const double us = u[(size_t)v * neq + idx];
            val = lin ? us : exp(us);
        } else {   // CHARGE
            double s = 0.0;
            for (int i = 0; i < ns; ++i) {
                const double ui = u[(size_t)v * neq + i];
                s += md->Z[i] * (lin ? ui : exp(ui));
            }
            val = FEDM_ELEMENTARY_CHARGE * s;
        }
        bad |= !isfinite(val);
    }
    dst[(size_t)k * nvp + v] = val;
    if (bad) atomicOr(flag, 1);
}

// out = first + num * (out - first) / den, file_output's expression, one rounding per operation
__global__ __launch_bounds__(FIELDS_THREADS) void fields_blend_kernel(size_t n, double num, double den,
                                                                      const double *__restrict__ first,
                                                                      double *__restrict__ out, int *__restrict__ flag) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = first[i], b = out[i];
    const double r = a + num * (b - a) / den;
    out[i] = r;
    if (!isfinite(r)) atomicOr(flag, 1);
}

// one vector's entries looked at for the flag (the result of a consistent solve)
__global__ __launch_bounds__(FIELDS_THREADS) void fields_finite_kernel(int n, const double *__restrict__ x,
                                                                       int *__restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !isfinite(x[i])) atomicOr(flag, 1);
}

// A thread per (request, point): sum_a w_a X[v_a], in that order
__global__ __launch_bounds__(FIELDS_THREADS) void fields_probe_kernel(int n_points, int n_req, int nvp,
                                                                      const int *__restrict__ p_vert,
                                                                      const double *__restrict__ p_w,
                                                                      const double *__restrict__ X,
                                                                      double *__restrict__ p_out) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_points * n_req) return;
    const int k = t / n_points, p = t - k * n_points;
    const double *Xk = X + (size_t)k * nvp;
    double s = 0.0;
    for (int a = 0; a < 3; ++a) s += p_w[3 * (size_t)p + a] * Xk[p_vert[3 * (size_t)p + a]];
    p_out[t] = s;
}

// ---- host ------------------------------------------------------------------------------------------
void fields_release(Ctx &c) {
    Fields *f = c.fields;
    if (!f) return;
    f->M.release();
    f->cg.release();
    void *ptrs[] = {f->v_ptr, f->v_idx, f->m, f->cell_b, f->out, f->first, f->flag, f->rhs, f->p_vert, f->p_w, f->p_out};
    for (void *p : ptrs)
        if (p) hipFree(p);
    if (f->h_out) hipHostFree(f->h_out);
    delete f;
    c.fields = nullptr;
}

namespace {

// the contexts the cell kernel is instantiated for (0), or the refusal
int check_ctx(const Ctx &c, const char *who) {
    if (c.model_kind != 0) return refuse(who, "the LMEA family has no field output (LFA models only)");
    if (!c.poisson && c.ns > 2)
        return refuse(who, std::to_string(c.ns) + " species without a Poisson equation: at most 2 are built");
    return 0;
}

int setup_impl(Ctx &c, const fedm_csr *mass, const char *who) {
    Fields &f = *c.fields;
    std::vector<int> cells((size_t)3 * c.nc);
    std::vector<double> coords((size_t)2 * c.nv);
    FEDM_HIP_CHECK(hipMemcpy(cells.data(), c.d_cells, sizeof(int) * cells.size(), hipMemcpyDeviceToHost));
    FEDM_HIP_CHECK(hipMemcpy(coords.data(), c.d_coords, sizeof(double) * coords.size(), hipMemcpyDeviceToHost));
    // vertex -> (cell, corner) in ascending order, and the lumped mass added in that order
    std::vector<int> v_ptr, v_idx;
    vertex_cell_lists(c.nv, cells, v_ptr, v_idx);
    std::vector<double> m((size_t)c.nvp, 0.0);
    for (int v = 0; v < c.nv; ++v) {
        double s = 0.0;
        for (int j = v_ptr[v]; j < v_ptr[v + 1]; ++j) {
            const int *cv = &cells[3 * (size_t)(v_idx[j] / 3)];
            const double *x0 = &coords[2 * (size_t)cv[0]], *x1 = &coords[2 * (size_t)cv[1]], *x2 = &coords[2 * (size_t)cv[2]];
            const double det = (x1[0] - x0[0]) * (x2[1] - x0[1]) - (x1[1] - x0[1]) * (x2[0] - x0[0]);
            s += std::fabs(det) / 6.0;
        }
        m[v] = s;
    }
    const size_t nvp = (size_t)c.nvp, K = FEDM_FIELDS_MAX_REQ;
    if (device_array(f.v_ptr, v_ptr.data(), v_ptr.size()) || device_array(f.v_idx, v_idx.data(), v_idx.size()) ||
        device_array(f.m, m.data(), m.size()) || device_array<double>(f.cell_b, nullptr, K * 3 * (size_t)c.nc) ||
        device_array<double>(f.out, nullptr, K * nvp) || device_array<double>(f.first, nullptr, K * nvp) ||
        device_array<int>(f.flag, nullptr, 1))
        return -1;
    FEDM_HIP_CHECK(hipHostMalloc((void **)&f.h_out, sizeof(double) * K * nvp));
    if (mass) {
        f.M.single = false;
        const int rc = f.M.from_csr(*mass, true);
        if (rc) {
            set_error(std::string(who) + ": mass matrix upload failed (bad CSR or out of memory)");
            return rc < -1 ? -2 : -1;
        }
        if (f.M.n_rows_p != c.nvp) return refuse(who, "the mass matrix's padded rows differ from the context's");
        if (device_array<double>(f.rhs, nullptr, nvp) || f.cg.alloc(nvp)) return -1;
        f.have_mass = true;
    }
    FEDM_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

bool projected(int kind) { return kind >= FEDM_FIELD_E_R && kind <= FEDM_FIELD_FLUX_Z; }

// the LFA family's cell and vertex pass: X(state) of every request into dst[n_req][nvp]
void launch_lfa(Ctx &c, const double *u, const FieldCellReqs &cq, const FieldVertexReqs &vq, int raw, double *dst) {
    Fields &f = *c.fields;
    const dim3 b(FIELDS_THREADS);
    if (cq.n > 0)
        with_model_flags(c, [&](auto ns, auto po, auto tab) {
            constexpr int NS = decltype(ns)::value;
            constexpr bool PO = decltype(po)::value, TAB = decltype(tab)::value;
            hipLaunchKernelGGL((fields_cell_kernel<NS, PO, TAB>), dim3((c.nc + FIELDS_THREADS - 1) / FIELDS_THREADS), b, 0,
                               c.stream, c.nc, c.d_model, c.d_coords, c.d_cells, u, cq, f.cell_b);
        });
    hipLaunchKernelGGL(fields_vertex_kernel, dim3((c.nvp + FIELDS_THREADS - 1) / FIELDS_THREADS, vq.n), b, 0, c.stream,
                       c.n_owned, c.nvp, c.nc, c.ns, c.neq, c.d_model, u, f.v_ptr, f.v_idx, f.m, f.cell_b, vq, raw, dst,
                       f.flag);
}

// X(state) of every request into dst[n_req][nvp].  Returns 0, or FEDM_DIVERGED_LINEAR when a solve stopped at max_it.
int evaluate(Ctx &c, const double *u, int n_req, const int *slot, const FieldsLaunch &launch, const fedm_field_opts &o,
             double *dst, int *its) {
    Fields &f = *c.fields;
    const dim3 b(FIELDS_THREADS);
    const int raw = o.projection == 1 ? 1 : 0;
    launch(u, raw, dst);
    int rc = 0;
    if (raw) {
        // the load vector of request k sits in dst[k]: it moves to rhs, and dst[k] becomes the solution from 0
        for (int k = 0; k < n_req; ++k) {
            if (slot[k] < 0) continue;
            double *x = dst + (size_t)k * c.nvp;
            hipMemcpyAsync(f.rhs, x, sizeof(double) * c.nvp, hipMemcpyDeviceToDevice, c.stream);
            hipMemsetAsync(x, 0, sizeof(double) * c.nvp, c.stream);
            const ScalarCgResult cg = scalar_pcg(c, f.cg, f.M, nullptr, f.rhs, x, o.rtol, o.max_it);
            its[k] += cg.it;
            const int status = cg.status(o.rtol);
            if (status == FEDM_DIVERGED_NAN) hipMemsetAsync(f.flag, 0xff, sizeof(int), c.stream);
            else if (status == FEDM_DIVERGED_LINEAR) rc = status;
            hipLaunchKernelGGL(fields_finite_kernel, dim3((c.nvp + FIELDS_THREADS - 1) / FIELDS_THREADS), b, 0, c.stream,
                               c.nvp, x, f.flag);
        }
    }
    return rc;
}

}  // namespace

int fields_setup_shared(Ctx &c, const fedm_csr *mass, const char *who) {
    if (mass) {
        if (c.n_owned != c.nv)
            return refuse(who, "the consistent projection runs on one GPU (this context has ghost vertices): no mass matrix");
        if (mass->n_rows != c.nv || mass->n_cols != c.nv || !mass->indptr || !mass->indices || !mass->values)
            return refuse(who, "the mass matrix has " + std::to_string(mass->n_rows) + " x " + std::to_string(mass->n_cols) +
                                   " entries, the mesh " + std::to_string(c.nv) + " vertices");
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    fields_release(c);
    c.fields = new Fields();
    const int rc = setup_impl(c, mass, who);
    if (rc != 0) fields_release(c);
    return rc;
}

int fields_probe_setup_shared(Ctx &c, int n_points, const int32_t *vertices, const double *weights, const char *who,
                              const char *setup_name) {
    if (!c.fields) return refuse(who, std::string(setup_name) + " has not been called");
    if (c.n_owned != c.nv) return refuse(who, "probes run on one GPU (this context has ghost vertices)");
    if (n_points < 0 || (n_points > 0 && (!vertices || !weights))) return refuse(who, "points without their arrays");
    for (int p = 0; p < n_points; ++p)
        for (int a = 0; a < 3; ++a) {
            const int v = vertices[3 * (size_t)p + a];
            if (v < 0 || v >= c.nv)
                return refuse(who, "vertex " + std::to_string(v) + " of point " + std::to_string(p) + " is out of range (the mesh has " +
                                       std::to_string(c.nv) + " vertices)");
            if (!std::isfinite(weights[3 * (size_t)p + a]))
                return refuse(who, "weight " + std::to_string(a) + " of point " + std::to_string(p) + " is not finite");
        }
    Fields &f = *c.fields;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    void *old[] = {f.p_vert, f.p_w, f.p_out};
    for (void *p : old)
        if (p) hipFree(p);
    f.p_vert = nullptr;
    f.p_w = nullptr;
    f.p_out = nullptr;
    f.n_points = 0;
    if (n_points == 0) return 0;
    if (device_array<int>(f.p_vert, vertices, (size_t)3 * n_points) || device_array<double>(f.p_w, weights, (size_t)3 * n_points) ||
        device_array<double>(f.p_out, nullptr, (size_t)FEDM_FIELDS_MAX_REQ * n_points))
        return -1;
    f.n_points = n_points;
    return 0;
}

int fields_check_opts(const Ctx &c, const fedm_field_opts &o, int n_req, const char *who, const char *setup_name) {
    if (!c.fields) return refuse(who, std::string(setup_name) + " has not been called");
    if (n_req < 1 || n_req > FEDM_FIELDS_MAX_REQ)
        return refuse(who, std::to_string(n_req) + " requests, 1 to " + std::to_string(FEDM_FIELDS_MAX_REQ) + " are possible");
    if (!std::isfinite(o.num) || !std::isfinite(o.den)) return refuse(who, "num or den of the blend is not finite");
    if (o.den == 0.0) return refuse(who, "den of the blend is 0");
    if (o.projection != 0 && o.projection != 1)
        return refuse(who, "projection " + std::to_string(o.projection) + ": 0 (lumped) or 1 (consistent)");
    if (!std::isfinite(o.rtol)) return refuse(who, "rtol is not finite");
    return 0;
}

int fields_check_projection(const Ctx &c, const fedm_field_opts &o, bool probes, const char *who, const char *setup_name,
                            const char *probe_name) {
    const Fields &f = *c.fields;
    if (o.projection == 1) {
        if (c.n_owned != c.nv) return refuse(who, "the consistent projection runs on one GPU (this context has ghost vertices)");
        if (!f.have_mass)
            return refuse(who, "the consistent projection needs the mass matrix of " + std::string(setup_name) + ", and none was given");
        if (!(o.rtol > 0.0) || o.max_it < 1) return refuse(who, "the consistent projection needs rtol > 0 and max_it >= 1");
    }
    if (probes && f.n_points == 0) return refuse(who, "probes asked for, and " + std::string(probe_name) + " has set no points");
    return 0;
}

int fields_run(Ctx &c, const fedm_field_opts &o, int n_req, const int *slot, bool any_projected, const FieldsLaunch &launch,
               double *nodal, double *probes, int32_t *finite, int32_t *cg_iterations) {
    Fields &f = *c.fields;
    const bool solve = o.projection == 1 && any_projected;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    const bool want_new = o.num != 0.0, want_old = o.num != o.den;
    if (want_new && c.halo_pending) {   // (several GPUs: the ghost entries of u_new are exchanged lazily)
        comm_halo(c, c.d_u);
        c.halo_pending = false;
    }
    fedm_field_opts o_run = o;
    if (!solve) o_run.projection = 0;   // (nothing projected: nothing to solve)
    int its[FEDM_FIELDS_MAX_REQ] = {0};
    FEDM_HIP_CHECK(hipMemsetAsync(f.flag, 0, sizeof(int), c.stream));
    int rc = 0;
    if (want_old && want_new) {
        rc = evaluate(c, c.d_uold, n_req, slot, launch, o_run, f.first, its);
        const int rc2 = evaluate(c, c.d_u, n_req, slot, launch, o_run, f.out, its);
        if (rc == 0) rc = rc2;
        const size_t n = (size_t)n_req * c.nvp;
        hipLaunchKernelGGL(fields_blend_kernel, dim3((unsigned)((n + FIELDS_THREADS - 1) / FIELDS_THREADS)),
                           dim3(FIELDS_THREADS), 0, c.stream, n, o.num, o.den, f.first, f.out, f.flag);
    } else {
        rc = evaluate(c, want_new ? c.d_u : c.d_uold, n_req, slot, launch, o_run, f.out, its);
    }
    if (probes) {
        const int n = f.n_points * n_req;
        hipLaunchKernelGGL(fields_probe_kernel, dim3((n + FIELDS_THREADS - 1) / FIELDS_THREADS), dim3(FIELDS_THREADS), 0,
                           c.stream, f.n_points, n_req, c.nvp, f.p_vert, f.p_w, f.out, f.p_out);
        FEDM_HIP_CHECK(hipMemcpyAsync(probes, f.p_out, sizeof(double) * n, hipMemcpyDeviceToHost, c.stream));
    }
    // the nodal results come down in one copy into pinned memory and are unpadded from there (a copy straight into the
    // caller's pageable rows measured 2.7 ms for two fields of 341 k vertices, next to 70 us of kernels)
    if (nodal)
        FEDM_HIP_CHECK(hipMemcpyAsync(f.h_out, f.out, sizeof(double) * n_req * c.nvp, hipMemcpyDeviceToHost, c.stream));
    int flag = 0;
    if (const int rc2 = read_result(c, flag, f.flag)) return rc2;
    for (int k = 0; nodal && k < n_req; ++k)
        std::memcpy(nodal + (size_t)k * c.nv, f.h_out + (size_t)k * c.nvp, sizeof(double) * c.nv);
    *finite = flag ? 0 : 1;
    if (cg_iterations)
        for (int k = 0; k < n_req; ++k) cg_iterations[k] = its[k];
    return rc;
}

}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_fields_setup(fedm_ctx *h, const fedm_csr *mass) {
    const char *who = "fedm_fields_setup";
    if (!h) return refuse(who, "null context");
    Ctx &c = h->c;
    if (const int rc = check_ctx(c, who)) return rc;
    return fields_setup_shared(c, mass, who);
}

int fedm_probe_setup(fedm_ctx *h, int n_points, const int32_t *vertices, const double *weights) {
    const char *who = "fedm_probe_setup";
    if (!h) return refuse(who, "null context");
    Ctx &c = h->c;
    if (const int rc = check_ctx(c, who)) return rc;
    return fields_probe_setup_shared(c, n_points, vertices, weights, who, "fedm_fields_setup");
}

int fedm_fields(fedm_ctx *h, const fedm_field_opts *opts, int n_req, const fedm_field_req *req, double *nodal,
                double *probes, int32_t *finite, int32_t *cg_iterations) {
    const char *who = "fedm_fields";
    if (!h || !opts || !req || !finite) return refuse(who, "null argument");
    Ctx &c = h->c;
    if (const int rc = check_ctx(c, who)) return rc;
    const fedm_field_opts &o = *opts;
    if (const int rc = fields_check_opts(c, o, n_req, who, "fedm_fields_setup")) return rc;
    FieldCellReqs cq{};
    FieldVertexReqs vq{};
    vq.n = n_req;
    for (int k = 0; k < n_req; ++k) {
        const int kind = req[k].kind, idx = req[k].index;
        const std::string r = "request " + std::to_string(k) + ": ";
        int limit = 1;   // indices 0 .. limit - 1
        switch (kind) {
            case FEDM_FIELD_STATE: limit = c.neq; break;
            case FEDM_FIELD_DENSITY:
            case FEDM_FIELD_FLUX_R:
            case FEDM_FIELD_FLUX_Z: limit = c.ns; break;
            case FEDM_FIELD_RATE: limit = c.model.n_reactions; break;
            case FEDM_FIELD_CHARGE:
            case FEDM_FIELD_E_R:
            case FEDM_FIELD_E_Z:
            case FEDM_FIELD_E_NORM: break;
            default: return refuse(who, r + "unknown kind " + std::to_string(kind));
        }
        if (idx < 0 || idx >= limit)
            return refuse(who, r + "index " + std::to_string(idx) + " out of range (0 to " + std::to_string(limit - 1) + ")");
        if (!c.poisson) {
            if (kind == FEDM_FIELD_E_R || kind == FEDM_FIELD_E_Z || kind == FEDM_FIELD_E_NORM)
                return refuse(who, r + "the field E needs a Poisson equation, and the model has none");
            if ((kind == FEDM_FIELD_FLUX_R || kind == FEDM_FIELD_FLUX_Z) &&
                c.model.eq_type[idx] == FEDM_EQ_DRIFT_DIFFUSION_REACTION && !c.model.has_drift_w[idx])
                return refuse(who, r + "the drift of species " + std::to_string(idx) +
                                       " needs E, hence a Poisson equation, and the model has none (no drift_w either)");
        }
        vq.kind[k] = kind;
        vq.index[k] = idx;
        vq.slot[k] = -1;
        if (projected(kind)) {
            vq.slot[k] = cq.n;
            cq.kind[cq.n] = kind;
            cq.index[cq.n] = idx;
            ++cq.n;
        }
    }
    if (const int rc = fields_check_projection(c, o, probes != nullptr, who, "fedm_fields_setup", "fedm_probe_setup")) return rc;
    return fields_run(c, o, n_req, vq.slot, cq.n > 0,
                      [&](const double *u, int raw_sums, double *dst) { launch_lfa(c, u, cq, vq, raw_sums, dst); }, nodal,
                      probes, finite, cg_iterations);
}

}  // extern "C"
