// C ABI of libfedm_hip.so (include/fedm_hip.h): the multigrid hierarchies of the potential block, built on the
// host from the caller's CSR levels (the composite operators of amg.hpp) and uploaded.
#include <algorithm>
#include <cstdlib>

#include "solver.hpp"

namespace fedm {

// ---- host-side sparse algebra for the composite multigrid levels (amg.hpp) ------------------
namespace {
struct HostCsr {
    int n_rows = 0, n_cols = 0;
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<double> values;
    fedm_csr view() const { return fedm_csr{n_rows, n_cols, indptr.data(), indices.data(), values.data()}; }
};

// alpha * A * diag(dc) * B  (dc may be null), rows merged with a dense accumulator, columns sorted
HostCsr csr_product(const fedm_csr &A, const double *dc, const fedm_csr &B, double alpha) {
    HostCsr out;
    out.n_rows = A.n_rows;
    out.n_cols = B.n_cols;
    out.indptr.assign((size_t)A.n_rows + 1, 0);
    std::vector<double> acc((size_t)B.n_cols, 0.0);
    std::vector<char> seen((size_t)B.n_cols, 0);
    std::vector<int32_t> cols;
    for (int i = 0; i < A.n_rows; ++i) {
        cols.clear();
        for (int64_t k = A.indptr[i]; k < A.indptr[i + 1]; ++k) {
            const int j = A.indices[k];
            const double a = alpha * A.values[k] * (dc ? dc[j] : 1.0);
            for (int64_t q = B.indptr[j]; q < B.indptr[j + 1]; ++q) {
                const int cidx = B.indices[q];
                if (!seen[cidx]) {
                    seen[cidx] = 1;
                    cols.push_back(cidx);
                }
                acc[cidx] += a * B.values[q];
            }
        }
        std::sort(cols.begin(), cols.end());
        for (int32_t cidx : cols) {
            out.indices.push_back(cidx);
            out.values.push_back(acc[cidx]);
            acc[cidx] = 0.0;
            seen[cidx] = 0;
        }
        out.indptr[i + 1] = (int64_t)out.indices.size();
    }
    return out;
}

// diag(dl) * (alpha * A + beta * B) with B's columns shifted by `shift` into a matrix of n_cols
// columns (A and B may overlap in pattern when shift == 0); dl may be null
HostCsr csr_combine(const fedm_csr &A, double alpha, const fedm_csr &B, double beta, int shift, int n_cols,
                    const double *dl) {
    HostCsr out;
    out.n_rows = A.n_rows;
    out.n_cols = n_cols;
    out.indptr.assign((size_t)A.n_rows + 1, 0);
    std::vector<std::pair<int32_t, double>> row;
    for (int i = 0; i < A.n_rows; ++i) {
        row.clear();
        const double s = dl ? dl[i] : 1.0;
        for (int64_t k = A.indptr[i]; k < A.indptr[i + 1]; ++k) row.emplace_back(A.indices[k], s * alpha * A.values[k]);
        for (int64_t k = B.indptr[i]; k < B.indptr[i + 1]; ++k)
            row.emplace_back(B.indices[k] + shift, s * beta * B.values[k]);
        std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (size_t k = 0; k < row.size(); ++k) {
            if (!out.indices.empty() && (int64_t)out.indices.size() > out.indptr[i] && out.indices.back() == row[k].first)
                out.values.back() += row[k].second;
            else {
                out.indices.push_back(row[k].first);
                out.values.push_back(row[k].second);
            }
        }
        out.indptr[i + 1] = (int64_t)out.indices.size();
    }
    return out;
}

HostCsr csr_identity(int n) {
    HostCsr out;
    out.n_rows = out.n_cols = n;
    out.indptr.resize((size_t)n + 1);
    out.indices.resize(n);
    out.values.assign(n, 1.0);
    for (int i = 0; i <= n; ++i) out.indptr[i] = i;
    for (int i = 0; i < n; ++i) out.indices[i] = i;
    return out;
}
}  // namespace

}  // namespace fedm

using namespace fedm;

extern "C" int fedm_amg_clear(fedm_ctx *h) {
    Ctx &c = h->c;
    if (c.amg || c.amg_alt) {
        hipSetDevice(c.device);
        set_hard_mode(c, false);
        hipStreamSynchronize(c.stream);
        iter_graphs_clear(c);
        for (Amg **a : {&c.amg, &c.amg_alt})
            if (*a) {
                (*a)->release();
                delete *a;
                *a = nullptr;
            }
    }
    return 0;
}

// shared by the rank-local hierarchy, the replicated global one (several GPUs) and the photoionisation terms (solver.hpp)
int fedm::build_amg(Ctx &c, int n_first_rows, int n_levels, const fedm_csr *A, const fedm_csr *P,
                    const fedm_csr *R, const double *coarse_inverse, int nu, double omega, Amg **out,
                    int composite_from, const double *poly_w) {
    // the hierarchy's matrices in single precision (FEDM_MG_F32=0: double); see EllMat::single
    const char *mg_env = std::getenv("FEDM_MG_F32");
    const bool mg_single = !(mg_env && mg_env[0] == '0');
    if (n_levels < 1 || !A || (n_levels > 1 && (!P || !R)) || nu == 0) {
        set_error("bad multigrid description");
        return -2;
    }
    if (A[0].n_rows != n_first_rows || A[0].n_cols != n_first_rows) {
        set_error("finest multigrid operator has the wrong size");
        return -2;
    }
    for (int l = 0; l + 1 < n_levels; ++l)
        if (P[l].n_rows != A[l].n_rows || P[l].n_cols != A[l + 1].n_rows ||
            R[l].n_rows != A[l + 1].n_rows || R[l].n_cols != A[l].n_rows) {
            set_error("inconsistent multigrid level shapes");
            return -2;
        }
    Amg *amg = new Amg();
    amg->nu = nu < 0 ? -nu : nu;  // nu < 0 selects V(0,|nu|) cycles
    amg->pre_smooth = nu > 0;
    amg->omega = omega;
    amg->poly = poly_w != nullptr;
    amg->levels.resize(n_levels);
    auto fail = [&](int rc) {
        amg->release();
        delete amg;
        return rc;
    };
    for (int l = 0; l < n_levels; ++l) {
        Amg::Level &L = amg->levels[l];
        int rc = 0;
        const char *composite_env = std::getenv("FEDM_AMG_COMPOSITE");  // "0": four kernels per level everywhere
        const bool composite_ok = !(composite_env && composite_env[0] == '0');
        L.composite = composite_ok && l + 1 < n_levels && l >= composite_from && (nu == 1 || poly_w);
        if (poly_w && l + 1 < n_levels) {
            // polynomial smoother: S_pre (weights in order), S_post (backwards), built by the
            // recurrence S <- S + w Dinv (I - A S) from S = w_0 Dinv
            const int n = A[l].n_rows, np = ((n + SLICE - 1) / SLICE) * SLICE;
            std::vector<double> dinv((size_t)n, 1.0);
            for (int i = 0; i < n; ++i)
                for (int64_t k = A[l].indptr[i]; k < A[l].indptr[i + 1]; ++k)
                    if (A[l].indices[k] == i && A[l].values[k] != 0.0) dinv[i] = 1.0 / A[l].values[k];
            const HostCsr I = csr_identity(n);
            const fedm_csr Iv = I.view();
            L.w.assign(poly_w + (size_t)l * nu, poly_w + (size_t)(l + 1) * nu);
            auto smoother = [&](const std::vector<double> &ws) {
                HostCsr S = csr_identity(n);
                for (int i = 0; i < n; ++i) S.values[i] = ws[0] * dinv[i];
                std::vector<double> wd((size_t)n);
                for (size_t k = 1; k < ws.size(); ++k) {
                    const HostCsr AS = csr_product(A[l], nullptr, S.view(), 1.0);
                    const HostCsr T = csr_combine(Iv, 1.0, AS.view(), -1.0, 0, n, nullptr);  // I - A S
                    for (int i = 0; i < n; ++i) wd[i] = ws[k] * dinv[i];
                    const HostCsr WT = csr_combine(T.view(), 1.0, T.view(), 0.0, 0, n, wd.data());
                    S = csr_combine(S.view(), 1.0, WT.view(), 1.0, 0, n, nullptr);
                }
                return S;
            };
            const HostCsr Spre = smoother(L.w);
            const HostCsr ASp = csr_product(A[l], nullptr, Spre.view(), 1.0);
            const HostCsr Tpre = csr_combine(Iv, 1.0, ASp.view(), -1.0, 0, n, nullptr);         // I - A S_pre
            const HostCsr Cm = csr_product(R[l], nullptr, Tpre.view(), 1.0);                     // R (I - A S_pre)
            L.C.single = mg_single;
            rc |= L.C.from_csr(Cm.view(), false);
            if (L.composite) {
                const HostCsr Spost = smoother(std::vector<double>(L.w.rbegin(), L.w.rend()));
                const HostCsr SA = csr_product(Spost.view(), nullptr, A[l], 1.0);
                const HostCsr E = csr_combine(Iv, 1.0, SA.view(), -1.0, 0, n, nullptr);          // I - S_post A
                const HostCsr ES = csr_product(E.view(), nullptr, Spre.view(), 1.0);
                const HostCsr G = csr_combine(ES.view(), 1.0, Spost.view(), 1.0, 0, n, nullptr);  // E S_pre + S_post
                const HostCsr Q = csr_product(E.view(), nullptr, P[l], 1.0);                       // E P
                const HostCsr GQ = csr_combine(G.view(), 1.0, Q.view(), 1.0, np, np + P[l].n_cols, nullptr);
                L.GQ.single = mg_single;
            rc |= L.GQ.from_csr(GQ.view(), false);
                L.A.n_rows = n;
                L.A.n_rows_p = np;
            } else {
                // leg up as one product on the concatenated vector [b ; x_c]: x = S b + P x_c
                const HostCsr SP = csr_combine(Spre.view(), 1.0, P[l], 1.0, np, np + P[l].n_cols, nullptr);
                L.A.single = mg_single;
            rc |= L.A.from_csr(A[l], true);
                L.S.single = mg_single;
            rc |= L.S.from_csr(SP.view(), false);
                L.down_composite = true;
            }
        } else if (L.composite) {
            const int n = A[l].n_rows, np = ((n + SLICE - 1) / SLICE) * SLICE;
            std::vector<double> wd((size_t)n, omega);  // w / A_ii (EllMat::from_csr's rule for dinv)
            for (int i = 0; i < n; ++i)
                for (int64_t k = A[l].indptr[i]; k < A[l].indptr[i + 1]; ++k)
                    if (A[l].indices[k] == i && A[l].values[k] != 0.0) wd[i] = omega / A[l].values[k];
            const HostCsr I = csr_identity(n);
            const fedm_csr Iv = I.view();
            const HostCsr M1 = csr_product(A[l], wd.data(), Iv, 1.0);                         // w A Dinv
            const HostCsr T = csr_combine(Iv, 1.0, M1.view(), -1.0, 0, n, nullptr);            // I - w A Dinv
            const HostCsr Cm = csr_product(R[l], nullptr, T.view(), 1.0);                      // R (I - w A Dinv)
            const HostCsr G = csr_combine(Iv, 2.0, M1.view(), -1.0, 0, n, wd.data());          // w Dinv (2I - w A Dinv)
            HostCsr WAP = csr_product(A[l], nullptr, P[l], 1.0);                               // w Dinv A P
            for (int i = 0; i < n; ++i)
                for (int64_t k = WAP.indptr[i]; k < WAP.indptr[i + 1]; ++k) WAP.values[k] *= wd[i];
            const HostCsr Q = csr_combine(P[l], 1.0, WAP.view(), -1.0, 0, P[l].n_cols, nullptr);  // (I - w Dinv A) P
            const HostCsr GQ = csr_combine(G.view(), 1.0, Q.view(), 1.0, np, np + P[l].n_cols, nullptr);
            L.C.single = mg_single;
            rc |= L.C.from_csr(Cm.view(), false);
            L.GQ.single = mg_single;
            rc |= L.GQ.from_csr(GQ.view(), false);
            L.A.n_rows = n;
            L.A.n_rows_p = np;
        } else if (l + 1 < n_levels) {
            L.A.single = mg_single;
            rc |= L.A.from_csr(A[l], true);
            L.P.single = mg_single;
            rc |= L.P.from_csr(P[l], false);
            // single-GPU hierarchy (its coarsest level is solved here): the finest level's leg down
            // as one product; across GPUs that level is a distributed operator with halo exchanges
            L.down_composite = composite_ok && l == 0 && composite_from == 1 && coarse_inverse && nu == 1;
            if (L.down_composite) {
                const int n = A[l].n_rows;
                std::vector<double> wd((size_t)n, omega);
                for (int i = 0; i < n; ++i)
                    for (int64_t k = A[l].indptr[i]; k < A[l].indptr[i + 1]; ++k)
                        if (A[l].indices[k] == i && A[l].values[k] != 0.0) wd[i] = omega / A[l].values[k];
                const HostCsr I = csr_identity(n);
                const HostCsr M1 = csr_product(A[l], wd.data(), I.view(), 1.0);
                const HostCsr T = csr_combine(I.view(), 1.0, M1.view(), -1.0, 0, n, nullptr);
                const HostCsr Cm = csr_product(R[l], nullptr, T.view(), 1.0);
                L.C.single = mg_single;
            rc |= L.C.from_csr(Cm.view(), false);
            } else {
                L.R.single = mg_single;
            rc |= L.R.from_csr(R[l], false);
            }
        } else {
            L.A.n_rows = A[l].n_rows;
            L.A.n_rows_p = ((A[l].n_rows + SLICE - 1) / SLICE) * SLICE;
        }
        if (rc) {
            set_error("multigrid level upload failed (bad CSR or out of memory)");
            return fail(rc < -1 ? -2 : -1);
        }
        const size_t n = (size_t)L.A.n_rows_p;
        const bool tail = L.composite || (poly_w && l + 1 < n_levels);  // b = [b ; next level's x]
        const size_t n_next = tail ? (size_t)(((A[l + 1].n_rows + SLICE - 1) / SLICE) * SLICE) : 0;
        L.x_is_alias = l > 0 && (amg->levels[l - 1].composite || poly_w);
        if (L.x_is_alias) L.x = amg->levels[l - 1].b + amg->levels[l - 1].A.n_rows_p;
        for (double **p : {&L.x, &L.x2, &L.b, &L.r}) {
            if (p == &L.x && L.x_is_alias) continue;
            const size_t len = n + (p == &L.b ? n_next : 0);
            if (hipMalloc((void **)p, sizeof(double) * len) != hipSuccess ||
                hipMemset(*p, 0, sizeof(double) * len) != hipSuccess) {
                set_error("out of device memory for the multigrid vectors");
                return fail(-1);
            }
        }
    }
    if (!coarse_inverse && composite_from == 1 && n_levels > 1 && c.n_owned < c.nv) {
        // several GPUs: which slices of the finest operator touch ghost columns
        const EllMat &A0 = amg->levels[0].A;
        const int l2s = A0.log2_split;
        std::vector<int> in_list, bd_list;
        for (int sl = 0; sl < A0.n_slices; ++sl) {
            bool ghost = false;
            for (int lane = 0; lane < SLICE && !ghost; lane += (1 << l2s)) {
                const int64_t r = ((int64_t)sl * SLICE + lane) >> l2s;
                if (r >= A[0].n_rows) break;
                for (int64_t k = A[0].indptr[r]; k < A[0].indptr[r + 1]; ++k)
                    if (A[0].indices[k] >= c.n_owned) {
                        ghost = true;
                        break;
                    }
            }
            (ghost ? bd_list : in_list).push_back(sl);
        }
        amg->n_interior0 = (int)in_list.size();
        amg->n_boundary0 = (int)bd_list.size();
        if (hipMalloc((void **)&amg->d_interior0, sizeof(int) * std::max<size_t>(in_list.size(), 1)) != hipSuccess ||
            hipMalloc((void **)&amg->d_boundary0, sizeof(int) * std::max<size_t>(bd_list.size(), 1)) != hipSuccess ||
            hipMemcpy(amg->d_interior0, in_list.data(), sizeof(int) * in_list.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(amg->d_boundary0, bd_list.data(), sizeof(int) * bd_list.size(), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("out of device memory for the multigrid slice lists");
            return fail(-1);
        }
    }
    amg->n_coarse = A[n_levels - 1].n_rows;
    amg->coarse_ld = ((amg->n_coarse + 255) / 256) * 256;
    if (coarse_inverse) {  // nullptr: the coarsest problem will be handed to a global hierarchy
        if (amg->n_coarse > 8192) {
            set_error("dense coarsest multigrid level above 8192 unknowns");
            return fail(-2);
        }
        std::vector<double> inv((size_t)amg->n_coarse * amg->coarse_ld, 0.0);
        for (int i = 0; i < amg->n_coarse; ++i)
            for (int j = 0; j < amg->n_coarse; ++j)
                inv[(size_t)i * amg->coarse_ld + j] = coarse_inverse[(size_t)i * amg->n_coarse + j];
        if (hipMalloc((void **)&amg->coarse_inv, sizeof(double) * inv.size()) != hipSuccess ||
            hipMemcpy(amg->coarse_inv, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("out of device memory for the coarse inverse");
            return fail(-1);
        }
    }
    *out = amg;
    return 0;
}

extern "C" {

int fedm_amg_setup(fedm_ctx *h, int n_levels, const fedm_csr *A, const fedm_csr *P,
                   const fedm_csr *R, const double *coarse_inverse, int nu, double omega) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    fedm_amg_clear(h);
    Amg *amg = nullptr;
    if (int rc = build_amg(c, c.nv, n_levels, A, P, R, coarse_inverse, nu, omega, &amg, 1)) return rc;
    c.amg = amg;
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (coarse_inverse && amg->capture(c) != 0) {
        hipGetLastError();  // graph capture unavailable: fall back to plain launches
    }
    return 0;
}

int fedm_amg_setup_poly(fedm_ctx *h, int n_levels, const fedm_csr *A, const fedm_csr *P, const fedm_csr *R,
                        const double *coarse_inverse, int degree, const double *weights, int as_alternative) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (degree < 1 || degree > 4 || !weights || !coarse_inverse || n_levels < 2) {
        set_error("polynomial-smoother hierarchy: degree 1..4, one weight per sweep and level, dense coarsest level");
        return -2;
    }
    for (int i = 0; i < (n_levels - 1) * degree; ++i)
        if (!(weights[i] > 0.0 && weights[i] < 8.0)) {
            set_error("polynomial-smoother weights must be positive");
            return -2;
        }
    if (c.comm) {
        set_error("polynomial-smoother hierarchy is for one GPU (the distributed finest level keeps V(1,1))");
        return -2;
    }
    if (as_alternative && !c.amg) {
        set_error("install the main hierarchy (fedm_amg_setup) before its alternative");
        return -2;
    }
    if (as_alternative) {
        set_hard_mode(c, false);
        if (c.amg_alt) {
            c.amg_alt->release();
            delete c.amg_alt;
            c.amg_alt = nullptr;
        }
    } else {
        fedm_amg_clear(h);
    }
    Amg *amg = nullptr;
    if (int rc = build_amg(c, c.nv, n_levels, A, P, R, coarse_inverse, degree, 1.0, &amg, 1, weights)) return rc;
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    (as_alternative ? c.amg_alt : c.amg) = amg;
    if (amg->capture(c) != 0) hipGetLastError();  // graph capture unavailable: plain launches
    return 0;
}

int fedm_amg_set_global_hierarchy(fedm_ctx *h, int n_global, int offset, int n_levels, const fedm_csr *A,
                                  const fedm_csr *P, const fedm_csr *R, const double *coarse_inverse,
                                  int nu, double omega) {
    Ctx &c = h->c;
    if (!c.amg || !coarse_inverse || offset < 0 || offset + c.amg->n_coarse > n_global) {
        set_error("bad global hierarchy description (install the local hierarchy first)");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    iter_graphs_clear(c);
    Amg &a = *c.amg;
    if (a.global) {
        a.global->release();
        delete a.global;
        a.global = nullptr;
    }
    if (a.graph_exec) {  // a captured cycle would solve the coarsest problem locally
        hipGraphExecDestroy(a.graph_exec);
        a.graph_exec = nullptr;
    }
    Amg *g = nullptr;
    if (int rc = build_amg(c, n_global, n_levels, A, P, R, coarse_inverse, nu, omega, &g, 0)) return rc;
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (g->capture(c) != 0) hipGetLastError();
    a.global = g;
    a.n_global = n_global;
    a.g_offset = offset;
    a.d_gb = g->levels[0].b;  // the global right-hand side IS the replicated hierarchy's input
    if (c.comm && comm_reserve_reduction(c, n_global)) return -1;
    return 0;
}

}  // extern "C"
