// Dielectric layers on boundary tags of an LFA model (include/fedm_hip.h, "dielectric-coated electrodes"): the part of
// the Poisson row that is no mirror of a species' wall term, the accept pass and the totals.  The mirror itself -- every
// facet term of a species row once more in the Poisson row, times -kappa Z_s -- is made where the facet terms are
// placed (boundary.hip, "Where boundary_facet's terms go"), with the wall formulas of element.hpp as they are.
//   layer_robin_kernel    per tagged facet of a layer: sum_q W_q (epsr/d)(Phi_q - U) phi_a into F and, with the
//                         Jacobian, (epsr/d) sum_q W_q phi_a phi_b into the (Phi, Phi) plane
//   layer_history_kernel  per layer vertex: -(1/eps0) [(1 + w)^2 q^n - w^2 q^(n-1)]/(1 + 2w) into F
//   layer_accept_kernel   per tagged facet, colour by colour without atomics: sum_s Z_s W_a,s(u) per layer vertex, by
//                         boundary_facet with a sink of its own; layer_shift_kernel then moves the history
//   layer_totals_kernel   one workgroup, fixed order: sum q_a and the displacement charge per tag
#include "dielectric.hpp"

#include <cmath>
#include <cstring>
#include <vector>

#include "element.hpp"
#include "postproc.hpp"
#include "solver.hpp"

namespace fedm {
namespace {

constexpr double EPS0 = FEDM_VACUUM_PERMITTIVITY;

// the two vertices of local facet fi, in the facet kernels' order
__device__ __forceinline__ void facet_ends(int fi, int &j, int &k) {
    j = (fi == 0) ? 1 : 0;
    k = (fi == 2) ? 1 : 2;
}

// The facet as the Robin term and the displacement charge see it: its cell's vertices, the potential there, the
// measure's r at the two ends and the length
struct LayerFacet {
    int v[3], j, k;
    double phi_j, phi_k, r_j, r_k, L;
    __device__ __forceinline__ void load(const fedm_model_desc *__restrict__ md, const int *__restrict__ cells,
                                         const double *__restrict__ coords, const double *__restrict__ u, int neq, int c,
                                         int fi) {
        facet_ends(fi, j, k);
        for (int a = 0; a < 3; ++a) v[a] = cells[3 * c + a];
        const double xj = coords[2 * v[j]], yj = coords[2 * v[j] + 1], xk = coords[2 * v[k]], yk = coords[2 * v[k] + 1];
        L = sqrt((xj - xk) * (xj - xk) + (yj - yk) * (yj - yk));
        r_j = md->axisymmetric ? xj : 0.5 / 3.14159265358979323846;
        r_k = md->axisymmetric ? xk : 0.5 / 3.14159265358979323846;
        phi_j = u[(size_t)v[j] * neq + neq - 1];
        phi_k = u[(size_t)v[k] * neq + neq - 1];
    }
};

template <bool ATOMIC>
__global__ void layer_robin_kernel(const fedm_model_desc *__restrict__ md, LayerTags lt, int n_facets,
                                   const int *__restrict__ facets, const int *__restrict__ cells,
                                   const double *__restrict__ coords, const uint32_t *__restrict__ cell_slots,
                                   const double *__restrict__ u, double *__restrict__ val, double *__restrict__ F, int neq,
                                   int jacobian) {
    const double two_pi = 6.283185307179586476925286766559;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_facets) return;
    const int c = facets[3 * t], fi = facets[3 * t + 1], tag = facets[3 * t + 2];
    const double cT = lt.c[tag - 1];
    if (cT == 0.0) return;   // no layer
    LayerFacet f;
    f.load(md, cells, coords, u, neq, c, fi);
    double R[2] = {0.0, 0.0}, M[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int q = 0; q < md->n_fqp; ++q) {
        const double p[2] = {1.0 - md->fqp_t[q], md->fqp_t[q]};
        const double W = md->fqp_w[q] * f.L * two_pi * (f.r_j * p[0] + f.r_k * p[1]) * cT;
        const double dphi = f.phi_j * p[0] + f.phi_k * p[1] - lt.U[tag - 1];
        for (int a = 0; a < 2; ++a) {
            R[a] += W * dphi * p[a];
            for (int b = 0; b < 2; ++b) M[a][b] += W * p[a] * p[b];
        }
    }
    const int e[2] = {f.j, f.k}, ip = neq - 1;
    for (int a = 0; a < 2; ++a) {
        double *pf = &F[(size_t)f.v[e[a]] * neq + ip];
        if (ATOMIC) unsafeAtomicAdd(pf, R[a]);
        else *pf += R[a];
        if (!jacobian) continue;
        for (int b = 0; b < 2; ++b) {
            const uint32_t slot = cell_slots[(size_t)c * 9 + e[a] * 3 + e[b]];
            double *pv = &val[((size_t)(slot >> 6) * neq * neq + ip * neq + ip) * SLICE + (slot & 63)];
            if (ATOMIC) unsafeAtomicAdd(pv, M[a][b]);
            else *pv += M[a][b];
        }
    }
}

// F_Phi,a -= (a1 q_a - a2 q_old_a)/eps0: one writer per entry
__global__ void layer_history_kernel(int n_lv, const int *__restrict__ lv, const double *__restrict__ q,
                                     const double *__restrict__ q_old, double a1, double a2, double *__restrict__ F,
                                     int neq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lv) return;
    F[(size_t)lv[i] * neq + neq - 1] -= (a1 * q[i] - a2 * q_old[i]) / EPS0;
}

// Where boundary_facet's residual terms go in the accept pass: Z_s times the term of species row s into the layer
// vertex's sum (plain adds: the facets of a launch share no vertex); nothing of the Jacobian
struct AcceptSink {
    double *__restrict__ &acc;
    const int *__restrict__ &lv_index;
    const fedm_model_desc *__restrict__ &md;
    int (&v)[3];
    __device__ __forceinline__ void operator()(int a, int s, double value) const { acc[lv_index[v[a]]] += md->Z[s] * value; }
};
struct NoJacobian {
    __device__ __forceinline__ void operator()(int, int, int, int, double) const {}
};

template <int NS, bool TAB, bool WALL>
__global__ __launch_bounds__(128) void layer_accept_kernel(
    const fedm_model_desc *__restrict__ md, uint32_t layer_tags, int n_facets, const int *__restrict__ facets,
    const int *__restrict__ cells, const double *__restrict__ coords, const double *__restrict__ u,
    const int *__restrict__ lv_index, double *__restrict__ acc) {
    constexpr int NEQ = NS + 1;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_facets) return;
    const int c = facets[3 * t], fi = facets[3 * t + 1], tag = facets[3 * t + 2];
    if (!((layer_tags >> (tag - 1)) & 1u)) return;
    int v[3];
    double x[3][2], Uc[3][NEQ];
    for (int a = 0; a < 3; ++a) {
        v[a] = cells[3 * c + a];
        x[a][0] = coords[2 * v[a]];
        x[a][1] = coords[2 * v[a] + 1];
        for (int s = 0; s < NEQ; ++s) Uc[a][s] = u[(size_t)v[a] * NEQ + s];
    }
    AcceptSink addR{acc, lv_index, md, v};
    boundary_facet<NS, TAB, WALL>(md, x, Uc, fi, tag, false, addR, NoJacobian{});
}

// q_old <- q, q <- a1 q - a2 q_old + cdt acc
__global__ void layer_shift_kernel(int n_lv, double *__restrict__ q, double *__restrict__ q_old,
                                   const double *__restrict__ acc, double a1, double a2, double cdt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lv) return;
    const double qn = q[i], qo = q_old[i];
    q_old[i] = qn;
    q[i] = (a1 * qn - a2 * qo) + cdt * acc[i];
}

// out[t] = sum of q over the vertices that count for tag t + 1, out[FEDM_MAX_TAGS + t] = eps0 epsr/d int (Phi - U) 2 pi r ds
// over its facets: every thread its stride in ascending order, then block_sums' fixed order
__global__ __launch_bounds__(POST_THREADS) void layer_totals_kernel(
    const fedm_model_desc *__restrict__ md, LayerTags lt, int n_lv, const int8_t *__restrict__ lv_tag,
    const double *__restrict__ q, int n_facets, const int *__restrict__ facets, const int *__restrict__ cells,
    const double *__restrict__ coords, const double *__restrict__ u, int neq, double *__restrict__ out) {
    constexpr int K = 2 * FEDM_MAX_TAGS;
    const double two_pi = 6.283185307179586476925286766559;
    __shared__ double lds[K][POST_WAVES];
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int i = threadIdx.x; i < n_lv; i += POST_THREADS) {
        const int tg = lv_tag[i];
        const double qi = q[i];
#pragma unroll
        for (int k = 0; k < FEDM_MAX_TAGS; ++k) s[k] += (k == tg) ? qi : 0.0;
    }
    for (int t = threadIdx.x; t < n_facets; t += POST_THREADS) {
        const int tg = facets[3 * t + 2] - 1;
        const double cT = lt.c[tg];
        if (cT == 0.0) continue;
        LayerFacet f;
        f.load(md, cells, coords, u, neq, facets[3 * t], facets[3 * t + 1]);
        double d = 0.0;
        for (int qp = 0; qp < md->n_fqp; ++qp) {
            const double p0 = 1.0 - md->fqp_t[qp], p1 = md->fqp_t[qp];
            d += md->fqp_w[qp] * f.L * two_pi * (f.r_j * p0 + f.r_k * p1) * (f.phi_j * p0 + f.phi_k * p1 - lt.U[tg]);
        }
        d *= EPS0 * cT;
#pragma unroll
        for (int k = 0; k < FEDM_MAX_TAGS; ++k) s[FEDM_MAX_TAGS + k] += (k == tg) ? d : 0.0;
    }
    const double r = block_sums<K>(s, lds);
    if ((int)threadIdx.x < K) out[threadIdx.x] = r;
}

// [(1 + w)^2, w^2]/(1 + 2w) and dt (1 + w)/(1 + 2w) of the context's step
struct LayerStep {
    double a1, a2, cdt;
};
LayerStep layer_step(const Ctx &c) {
    const double w = c.dt / c.dt_old;
    return {(1.0 + w) * (1.0 + w) / (1.0 + 2.0 * w), w * w / (1.0 + 2.0 * w), c.dt * (1.0 + w) / (1.0 + 2.0 * w)};
}

// the refusal the per-context calls share
int layer_refusal(fedm_ctx *h, const char *who) {
    if (!h) return refuse(who, "null argument");
    if (h->c.model_kind != 0) return refuse(who, "the LMEA family has no dielectric layers (LFA models only)");
    if (!h->c.diel) return refuse(who, "this context has no dielectric layer (fedm_ctx_create_dielectric)");
    return 0;
}

// per-vertex caller arrays <-> the layer vertices' compact ones
int scatter_to_vertices(Ctx &c, const double *dev, double *out) {
    Dielectric &d = *c.diel;
    std::vector<double> h((size_t)d.n_lv);
    std::vector<int> lv((size_t)d.n_lv);
    FEDM_HIP_CHECK(hipMemcpy(h.data(), dev, sizeof(double) * d.n_lv, hipMemcpyDeviceToHost));
    FEDM_HIP_CHECK(hipMemcpy(lv.data(), d.lv, sizeof(int) * d.n_lv, hipMemcpyDeviceToHost));
    std::fill(out, out + c.nv, 0.0);
    for (int i = 0; i < d.n_lv; ++i) out[lv[i]] = h[i];
    return 0;
}
int gather_from_vertices(Ctx &c, const double *in, double *dev) {
    Dielectric &d = *c.diel;
    std::vector<double> h((size_t)d.n_lv);
    std::vector<int> lv((size_t)d.n_lv);
    FEDM_HIP_CHECK(hipMemcpy(lv.data(), d.lv, sizeof(int) * d.n_lv, hipMemcpyDeviceToHost));
    for (int i = 0; i < d.n_lv; ++i) h[i] = in[lv[i]];
    FEDM_HIP_CHECK(hipMemcpy(dev, h.data(), sizeof(double) * d.n_lv, hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

LayerMirror layer_mirror(const Ctx &c) {
    LayerMirror m = {};
    const double kappa = c.model.charge_over_eps * layer_step(c).cdt;
    for (int s = 0; s < c.ns; ++s) m.kz[s] = -kappa * c.model.Z[s];
    m.tags = c.diel->tags;
    return m;
}

LayerTags layer_tags(const Ctx &c) {
    LayerTags t = {};
    const fedm_dielectric_desc &d = c.diel->desc;
    for (int k = 0; k < FEDM_MAX_TAGS; ++k) {
        t.c[k] = d.is_layer[k] ? d.eps_r[k] / d.thickness[k] : 0.0;
        t.U[k] = d.voltage[k];
    }
    return t;
}

int dielectric_setup(Ctx &c, const fedm_dielectric_desc &desc, const fedm_mesh_desc &mesh, bool *dirichlet_on_layer) {
    Dielectric *d = new Dielectric();
    c.diel = d;
    d->desc = desc;
    for (int k = 0; k < FEDM_MAX_TAGS; ++k)
        if (desc.is_layer[k]) d->tags |= 1u << k;
    // the vertices of the layers' facets that lie on them, each with the lowest tag it was met under
    std::vector<int8_t> tag_of((size_t)c.nv, -1);
    for (int cell = 0; cell < c.nc && mesh.facet_tags; ++cell)
        for (int i = 0; i < 3; ++i) {
            const int tg = mesh.facet_tags[3 * cell + i] - 1;
            if (tg < 0 || !desc.is_layer[tg]) continue;
            for (int a = 0; a < 3; ++a) {
                if (a == i) continue;
                int8_t &t = tag_of[mesh.cells[3 * cell + a]];
                if (t < 0 || tg < t) t = (int8_t)tg;
            }
        }
    std::vector<int> lv, index((size_t)c.nv, -1);
    std::vector<int8_t> lv_tag;
    for (int v = 0; v < c.nv; ++v)
        if (tag_of[v] >= 0) {
            index[v] = (int)lv.size();
            lv.push_back(v);
            lv_tag.push_back(tag_of[v]);
        }
    d->n_lv = (int)lv.size();
    *dirichlet_on_layer = false;
    for (int k = 0; k < mesh.n_dirichlet; ++k) {
        const int dof = mesh.dirichlet_dofs[k];
        if (dof % c.neq == c.neq - 1 && tag_of[dof / c.neq] >= 0) *dirichlet_on_layer = true;
    }
    if (device_array<int>(d->lv, lv.data(), lv.size()) || device_array<int8_t>(d->lv_tag, lv_tag.data(), lv_tag.size()) ||
        device_array<int>(d->lv_index, index.data(), index.size()) || device_array<double>(d->q, nullptr, lv.size()) ||
        device_array<double>(d->q_old, nullptr, lv.size()) || device_array<double>(d->acc, nullptr, lv.size()) ||
        device_array<double>(d->totals, nullptr, 2 * FEDM_MAX_TAGS))
        return -1;
    return 0;
}

void dielectric_release(Ctx &c) {
    if (!c.diel) return;
    Dielectric &d = *c.diel;
    void *ptrs[] = {d.lv, d.lv_tag, d.lv_index, d.q, d.q_old, d.acc, d.totals};
    for (void *p : ptrs)
        if (p) hipFree(p);
    delete c.diel;
    c.diel = nullptr;
}

void launch_layer_rows(Ctx &c, bool jacobian, int mode) {
    Dielectric &d = *c.diel;
    const LayerTags lt = layer_tags(c);
    auto robin = [&](auto kernel, int f0, int n) {
        if (n > 0)
            hipLaunchKernelGGL(kernel, dim3((n + 127) / 128), dim3(128), 0, c.stream, c.d_model, lt, n, c.d_bfacets + 3 * f0,
                               c.d_cells, c.d_coords, c.d_cell_slots, c.d_u, c.d_val, c.d_F, c.neq, jacobian ? 1 : 0);
    };
    if (c.assembly_kind == 1) {
        robin(layer_robin_kernel<true>, 0, c.n_bfacets);
    } else {   // the colouring's fixed order: one launch per facet colour, plain adds
        for (size_t k = 0; k + 1 < c.bfacet_colour_ptr.size(); ++k)
            robin(layer_robin_kernel<false>, c.bfacet_colour_ptr[k], c.bfacet_colour_ptr[k + 1] - c.bfacet_colour_ptr[k]);
    }
    // Poisson row only: the species are frozen and with them the surface charge, at what was accepted last
    const LayerStep st = mode == 1 ? LayerStep{1.0, 0.0, 0.0} : layer_step(c);
    if (d.n_lv > 0)
        hipLaunchKernelGGL(layer_history_kernel, dim3((d.n_lv + 255) / 256), dim3(256), 0, c.stream, d.n_lv, d.lv, d.q,
                           d.q_old, st.a1, st.a2, c.d_F, c.neq);
}

}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_dielectric_set_voltage(fedm_ctx *h, const double U[FEDM_MAX_TAGS]) {
    const char *who = "fedm_dielectric_set_voltage";
    if (const int rc = layer_refusal(h, who)) return rc;
    if (!U) return refuse(who, "null argument");
    fedm_dielectric_desc &d = h->c.diel->desc;
    for (int k = 0; k < FEDM_MAX_TAGS; ++k)
        if (d.is_layer[k] && !std::isfinite(U[k])) return refuse(who, "the voltage of tag " + std::to_string(k + 1) + " is not finite");
    for (int k = 0; k < FEDM_MAX_TAGS; ++k)
        if (d.is_layer[k]) d.voltage[k] = U[k];
    return 0;
}

int fedm_dielectric_accept(fedm_ctx *h) {
    if (const int rc = layer_refusal(h, "fedm_dielectric_accept")) return rc;
    Ctx &c = h->c;
    Dielectric &d = *c.diel;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (d.n_lv == 0) return 0;
    FEDM_HIP_CHECK(hipMemsetAsync(d.acc, 0, sizeof(double) * d.n_lv, c.stream));
    with_model_flags(c, [&](auto ns, auto, auto tab) {
        constexpr int NS = decltype(ns)::value;
        constexpr bool TAB = decltype(tab)::value;
        for (size_t k = 0; k + 1 < c.bfacet_colour_ptr.size(); ++k) {
            const int f0 = c.bfacet_colour_ptr[k], n = c.bfacet_colour_ptr[k + 1] - f0;
            if (n <= 0) continue;
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3((n + 127) / 128), dim3(128), 0, c.stream, c.d_model, d.tags, n,
                                   c.d_bfacets + 3 * f0, c.d_cells, c.d_coords, c.d_u, d.lv_index, d.acc);
            };
            if (c.model_walls) launch(layer_accept_kernel<NS, TAB, true>);
            else launch(layer_accept_kernel<NS, TAB, false>);
        }
    });
    const LayerStep st = layer_step(c);
    const double e = c.model.charge_over_eps * EPS0;
    hipLaunchKernelGGL(layer_shift_kernel, dim3((d.n_lv + 255) / 256), dim3(256), 0, c.stream, d.n_lv, d.q, d.q_old, d.acc,
                       st.a1, st.a2, st.cdt * e);
    FEDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int fedm_dielectric_get(fedm_ctx *h, struct fedm_dielectric_totals *totals, double *q, double *q_old) {
    if (const int rc = layer_refusal(h, "fedm_dielectric_get")) return rc;
    Ctx &c = h->c;
    Dielectric &d = *c.diel;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (totals) {
        hipLaunchKernelGGL(layer_totals_kernel, dim3(1), dim3(POST_THREADS), 0, c.stream, c.d_model, layer_tags(c), d.n_lv,
                           d.lv_tag, d.q, c.n_bfacets, c.d_bfacets, c.d_cells, c.d_coords, c.d_u, c.neq, d.totals);
        double sums[2 * FEDM_MAX_TAGS];
        FEDM_HIP_CHECK(hipMemcpyAsync(sums, d.totals, sizeof(sums), hipMemcpyDeviceToHost, c.stream));
        FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
        FEDM_HIP_CHECK(hipGetLastError());
        *totals = {};
        for (int k = 0; k < FEDM_MAX_TAGS; ++k) {
            totals->charge[k] = sums[k];
            totals->displacement[k] = sums[FEDM_MAX_TAGS + k];
            totals->voltage[k] = d.desc.voltage[k];
        }
        totals->n_layer_vertices = d.n_lv;
    }
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (q && scatter_to_vertices(c, d.q, q)) return -1;
    if (q_old && scatter_to_vertices(c, d.q_old, q_old)) return -1;
    return 0;
}

int fedm_dielectric_set(fedm_ctx *h, const double *q, const double *q_old) {
    if (const int rc = layer_refusal(h, "fedm_dielectric_set")) return rc;
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (q && gather_from_vertices(c, q, c.diel->q)) return -1;
    if (q_old && gather_from_vertices(c, q_old, c.diel->q_old)) return -1;
    return 0;
}

}  // extern "C"
