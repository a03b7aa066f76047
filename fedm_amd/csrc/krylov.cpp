// The linear solvers behind the C ABI: GMRES (coupled system, species block) with its captured Krylov steps, and
// the preconditioned CG of the potential rows.  Host logic only; every flop runs in the kernels' sources.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <deque>

#include "solver.hpp"

namespace fedm {

// The switches of the Krylov loop, read once per process; each is on unless its variable begins with '0'.
struct KrylovSwitches {
    bool halo_overlap;        // FEDM_HALO_OVERLAP: the halo exchange of a step on the communication stream
    bool pairs;               // FEDM_KRYLOV_PAIRS: two steps as one graph
    bool skip_last_update;    // FEDM_KRYLOV_SKIP_LAST_UPDATE: the step expected to end a solve goes without its update
    bool first_by_producer;   // FEDM_FS_FIRST_BY_PRODUCER: see krylov_vector_update
};
static const KrylovSwitches &switches() {
    static const KrylovSwitches s = [] {
        auto on = [](const char *name) {
            const char *e = std::getenv(name);
            return !(e && e[0] == '0');
        };
        return KrylovSwitches{on("FEDM_HALO_OVERLAP"), on("FEDM_KRYLOV_PAIRS"), on("FEDM_KRYLOV_SKIP_LAST_UPDATE"),
                              on("FEDM_FS_FIRST_BY_PRODUCER")};
    }();
    return s;
}

// The least-squares problem of GMRES(m), min |beta e_1 - H y|: the Hessenberg matrix (row-major, H[i * m + j]) is
// kept triangular by one Givens rotation per column; g is the rotated right-hand side.
struct HessenbergLeastSquares {
    int m;
    std::vector<double> H, cs, sn, g, y;
    explicit HessenbergLeastSquares(int m_) : m(m_), H((size_t)(m_ + 1) * m_, 0.0), cs(m_), sn(m_), g(m_ + 1), y(m_) {}
    void reset(double beta) {
        std::fill(g.begin(), g.end(), 0.0);
        g[0] = beta;
    }
    // column j = (h[0..j], hn): the old rotations, then the new one; returns the recurrence's residual norm |g[j+1]|
    double add_column(int j, const double *h, double hn) {
        for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] = h[i];
        H[(size_t)(j + 1) * m + j] = hn;
        for (int i = 0; i < j; ++i) {
            const double t = cs[i] * H[(size_t)i * m + j] + sn[i] * H[(size_t)(i + 1) * m + j];
            H[(size_t)(i + 1) * m + j] = -sn[i] * H[(size_t)i * m + j] + cs[i] * H[(size_t)(i + 1) * m + j];
            H[(size_t)i * m + j] = t;
        }
        const double a = H[(size_t)j * m + j], b = H[(size_t)(j + 1) * m + j];
        const double d = std::hypot(a, b);
        cs[j] = d > 0.0 ? a / d : 1.0;
        sn[j] = d > 0.0 ? b / d : 0.0;
        H[(size_t)j * m + j] = d;
        H[(size_t)(j + 1) * m + j] = 0.0;
        g[j + 1] = -sn[j] * g[j];
        g[j] = cs[j] * g[j];
        return std::fabs(g[j + 1]);
    }
    // back substitution over the first k columns
    const double *solve(int k) {
        for (int i = k - 1; i >= 0; --i) {
            double s = g[i];
            for (int l = i + 1; l < k; ++l) s -= H[(size_t)i * m + l] * y[l];
            y[i] = s / H[(size_t)i * m + i];
        }
        return y.data();
    }
};

int ensure_krylov(Ctx &c, int restart) {
    if (ensure_spmv_dots(c)) return -1;
    if (restart + 1 <= c.krylov_cap) return 0;
    iter_graphs_clear(c);  // they hold the old Krylov vectors' addresses
    if (c.d_V) hipFree(c.d_V);
    c.d_V = nullptr;
    FEDM_HIP_CHECK(hipMalloc((void **)&c.d_V, sizeof(double) * (size_t)c.np * (restart + 1)));
    if (c.d_Z) hipFree(c.d_Z);
    c.d_Z = nullptr;
    FEDM_HIP_CHECK(hipMalloc((void **)&c.d_Z, sizeof(double) * (size_t)c.np * restart));
    c.krylov_cap = restart + 1;
    return 0;
}

// w = Minv (J v): point-block Jacobi (fused in the SpMV) or field split with multigrid
static void apply_operator(Ctx &c, const double *v, double *w) {
    comm_halo(c, const_cast<double *>(v));  // ghost inputs from their owners (multi-GPU)
    if (c.amg && c.poisson) {
        fieldsplit_apply_operator(c, *c.amg, v, c.d_tmp, w, true);
    } else {
        prof_begin(c, 1);
        launch_spmv(c, v, w, true);
        prof_end(c);
    }
}

// the field split sits on the right of the operator (flexible GMRES)
// (across GPUs always: the left variant is kept for one GPU only -- its restarted cycles were never
// made to work over several ranks)
bool right_preconditioned(const Ctx &c) { return (c.right_precond || c.comm) && c.amg && c.poisson; }

// rhs = -Minv F (preconditioner on the left) or -F (on the right), after the Jacobian has been assembled
void prepare_preconditioner_and_rhs(Ctx &c) {
    if (right_preconditioned(c)) {
        fieldsplit_setup(c);  // the right-hand side is -F itself: gmres reads c.d_F
    } else if (c.amg && c.poisson) {
        fieldsplit_setup(c);
        fieldsplit_apply(c, *c.amg, c.d_F, c.d_rhs, -1.0);
    } else {
        launch_block_inverse(c);
        launch_apply_dinv(c, c.d_F, c.d_rhs, -1.0);
    }
}

void iter_graphs_clear(Ctx &c) {
    for (auto *vec : {&c.iter_graph, &c.iter_graph_interior, &c.iter_graph_pre, &c.iter_graph_pair, &c.iter_graph_last,
                      &c.iter_graph_pair_last, &c.iter_graph_refined}) {
        for (hipGraphExec_t g : *vec)
            if (g) hipGraphExecDestroy(g);
        vec->clear();
    }
}

// Producers of Krylov vectors.  One GPU, field split on the right with species sweeps (Ctx::fs_first_by_producer, set by
// gmres): the kernel that completes v_j also forms the first stage of the preconditioner for it (cgs_update_fs_kernel).
void krylov_vector_update(Ctx &c, int k, const double *const *vp, double *w) {
    if (c.fs_first_by_producer) {
        if (!launch_cgs_update_fs(c, k, vp, w, reinterpret_cast<float *>(c.d_fs_g), c.amg->levels[0].b)) {
            launch_cgs_update(c, k, vp, w);
            fieldsplit_first_stage(c, *c.amg, w);
        }
    } else {
        launch_cgs_update(c, k, vp, w);
    }
}

void krylov_vector_scale(Ctx &c, double a, const double *x, double *y) {
    if (c.fs_first_by_producer) {
        if (!launch_scale_copy_fs(c, a, x, y, reinterpret_cast<float *>(c.d_fs_g), c.amg->levels[0].b)) {
            launch_scale_copy(c, a, x, y);
            fieldsplit_first_stage(c, *c.amg, y);
        }
    } else {
        launch_scale_copy(c, a, x, y);
    }
}

template <class Body>
static bool capture_graph(Ctx &c, hipGraphExec_t *out, Body &&body) {
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(c.stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        hipGetLastError();
        return false;
    }
    c.capturing = true;
    body();
    c.capturing = false;
    hipGraphExec_t exec = nullptr;
    const bool ok = hipStreamEndCapture(c.stream, &graph) == hipSuccess && graph &&
                    hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) hipGraphDestroy(graph);
    if (!ok) {
        hipGetLastError();
        return false;
    }
    *out = exec;
    return true;
}

// ---- what the captured and the plain Krylov steps share ------------------------------------------
// the operands of a step's dot products: {v_0 ... v_j, w}
static std::vector<const double *> dot_operands(const double *const *vp, int j, const double *w) {
    std::vector<const double *> dotp(vp, vp + j + 1);
    dotp.push_back(w);
    return dotp;
}

// While this lives the V-cycle's last sweep writes the potential component of `out` itself (`direct`: V(nu,nu) with
// more than one level); otherwise a reduction or scatter kernel does.
struct DirectOutput {
    Amg &amg;
    DirectOutput(Ctx &c, bool direct, double *out) : amg(*c.amg) {
        if (direct) {
            amg.out = out;
            amg.out_stride = c.neq;
            amg.out_offset = c.neq - 1;
        }
    }
    ~DirectOutput() { amg.out = nullptr; }
};

// w = J z with the dot products {v_0 ... v_j, w}.w: one kernel where it is instantiated, two otherwise
static void product_and_dots(Ctx &c, const double *z, double *w, const double *const *dotp, int n, bool publish) {
    if (!launch_spmv_dots(c, z, w, dotp, n, publish ? SPMV_DOTS_PUBLISH : SPMV_DOTS_SUMS)) {
        launch_spmv(c, z, w, false);
        launch_dots_fused(c, dotp, w, n, nullptr, publish);
    }
}

// false: the launch failed, and every later step runs with plain launches
static bool launch_graph(Ctx &c, hipGraphExec_t exec) {
    if (hipGraphLaunch(exec, c.stream) == hipSuccess) return true;
    hipGetLastError();
    c.iter_graphs_ok = false;
    return false;
}

// cache[j], captured the first time index j is reached, then launched; it publishes `publications` times
template <class Body>
static bool replay(Ctx &c, std::vector<hipGraphExec_t> &cache, int j, int publications, Body &&body) {
    if ((int)cache.size() <= j) cache.resize(j + 1, nullptr);
    if (!cache[j] && !capture_graph(c, &cache[j], body)) {
        c.iter_graphs_ok = false;
        return false;
    }
    if (!launch_graph(c, cache[j])) return false;
    c.mail_seq += publications;
    return true;
}

// several GPUs, after a step's graphs: the sums over the ranks, finish / publish, the next Krylov vector
static void reduce_and_update(Ctx &c, int j, const double *const *vp, double *w) {
    comm_allreduce(c, c.d_red, j + 2);
    launch_cgs_finish(c, j + 2);
    krylov_vector_update(c, j + 1, vp, w);
}

// w = J z (z complete on every rank), h = V^T w, w <- (w - V h)/|.| with plain launches
// (behind a failed graph launch the SpMV event is never recorded: graphs run only while that kind of event is off)
static void plain_product_and_update(Ctx &c, int j, const double *const *vp, double *z, double *w) {
    prof_begin(c, 1);
    launch_spmv(c, z, w, false);
    prof_end(c);
    launch_dots(c, dot_operands(vp, j, w).data(), w, j + 2, true);
    krylov_vector_update(c, j + 1, vp, w);
}

// One Krylov step  w = Minv J v_j;  h = V^T w;  w <- (w - V h)/|.|  as a hipGraph, captured the
// first time index j is reached: ~30 kernels replayed back to back with no launch gaps and one
// host call.  All pointers are fixed for a given j; the mailbox tag is a device counter.
// Across GPUs the collectives stay outside the graphs, and the halo exchange of v_j runs on the
// communication stream while the compute stream already multiplies the interior matrix slices
// (those without ghost columns):
//   mark v_j complete -> graph I_j (interior SpMV)  ||  exchange  -> wait -> graph B_j (boundary
//   SpMV, preconditioner, local partial sums) -> all-reduce -> finish/publish -> update.
static bool iter_graph_launch(Ctx &c, int j, const double *const *vp, double *w) {
    if (!c.iter_graphs_ok || !(c.amg && c.poisson) || (c.prof.on && c.prof.all_kinds)) return false;
    const bool multi = c.comm != nullptr;
    if ((int)c.iter_graph.size() <= j) {
        c.iter_graph.resize(j + 1, nullptr);
        c.iter_graph_interior.resize(j + 1, nullptr);
    }
    const std::vector<const double *> dotp = dot_operands(vp, j, w);
    if (!c.iter_graph[j]) {
        // the V-cycle's last sweep writes the potential component of w itself; otherwise the reduction kernel
        // scatters it
        const bool direct = c.amg->pre_smooth && c.amg->levels.size() > 1;
        const double *x0 = direct ? nullptr : c.amg->levels[0].x;
        bool ok = true;
        if (!multi) {
            ok = capture_graph(c, &c.iter_graph[j], [&] {
                {
                    DirectOutput out(c, direct, w);
                    fieldsplit_apply_operator(c, *c.amg, vp[j], c.d_tmp, w, false);
                }
                launch_dots_fused(c, dotp.data(), w, j + 2, x0, true);
                krylov_vector_update(c, j + 1, vp, w);
            });
        } else {
            Comm &cm = *c.comm;
            if (cm.n_interior)
                ok = capture_graph(c, &c.iter_graph_interior[j], [&] {
                    fieldsplit_apply_operator_part(c, *c.amg, vp[j], c.d_tmp, w, false, 0, cm.d_interior, cm.n_interior);
                });
            if (c.amg->global)  // the V-cycle contains collectives: the graph ends at its right-hand side
                ok = ok && capture_graph(c, &c.iter_graph[j], [&] {
                    fieldsplit_apply_operator_part(c, *c.amg, vp[j], c.d_tmp, w, false, 2, cm.d_boundary, cm.n_boundary);
                });
            else
                ok = ok && capture_graph(c, &c.iter_graph[j], [&] {
                    {
                        DirectOutput out(c, direct, w);
                        fieldsplit_apply_operator_part(c, *c.amg, vp[j], c.d_tmp, w, false, 1, cm.d_boundary, cm.n_boundary);
                    }
                    launch_dots_fused(c, dotp.data(), w, j + 2, x0, false);
                });
        }
        if (!ok) {
            c.iter_graphs_ok = false;
            return false;
        }
    }
    if (!multi) {
        if (!launch_graph(c, c.iter_graph[j])) return false;
        ++c.mail_seq;
        return true;
    }
    // FEDM_HALO_OVERLAP=0 keeps the exchange on the compute stream (diagnostics)
    const bool overlap = switches().halo_overlap;
    if (overlap) comm_halo_begin(c);
    else comm_halo(c, const_cast<double *>(vp[j]));
    bool ok = !c.iter_graph_interior[j] || launch_graph(c, c.iter_graph_interior[j]);
    if (overlap) comm_halo_exchange(c, const_cast<double *>(vp[j]));
    ok = ok && launch_graph(c, c.iter_graph[j]);
    if (!ok) {  // the exchange has happened: redo the whole step with plain launches (same result)
        fieldsplit_apply_operator(c, *c.amg, vp[j], c.d_tmp, w, true);
        launch_dots(c, dotp.data(), w, j + 2, true);
        krylov_vector_update(c, j + 1, vp, w);
        return true;
    }
    if (c.amg->global) {  // V-cycle with its collectives, then scatter + local partial sums
        c.amg->run(c);
        launch_dots_fused(c, dotp.data(), w, j + 2, c.amg->levels[0].x, false);
    }
    reduce_and_update(c, j, vp, w);
    return true;
}

// The same step with the field split on the right:  z_j = Minv v_j (kept),  w = J z_j,  h = V^T w,
// w <- (w - V h)/|.|.  One GPU: one graph.  Several GPUs: it is z_j whose ghost entries the
// product needs --
//   graph P_j (first stage, sweeps, coupling[, V-cycle]) [-> V-cycle with its collectives] ->
//   mark z_j complete -> graph I_j (interior rows of J z_j)  ||  exchange of z_j -> wait ->
//   graph B_j (boundary rows, local partial sums) -> all-reduce -> finish/publish -> update.
// The Krylov vectors keep zero ghost entries (ghost rows of the product are zero), so Minv sees
// the same inputs as on the left.
// (deep halos exchange v_j, the step's input, on all ghost layers instead: `exchanged` says that the caller has)
static void right_step_plain(Ctx &c, int j, const double *const *vp, double *z, double *w, bool exchanged) {
    const bool deep = deep_halo_active(c);
    if (deep && !exchanged) comm_halo(c, const_cast<double *>(vp[j]));
    fieldsplit_apply(c, *c.amg, vp[j], z, 1.0);
    if (!deep) comm_halo(c, z);
    plain_product_and_update(c, j, vp, z, w);
}

// the V-cycle's last sweep writes the potential component of z itself (V(nu,nu) with more than one level); otherwise a
// scatter kernel does.  Upper-triangular order: the V-cycle comes first and the last species sweep writes the whole of z.
static bool right_direct_output(const Ctx &c) {
    return !fieldsplit_upper(c) && c.amg->pre_smooth && c.amg->levels.size() > 1;
}

// what a one-GPU graph records for step j; `update` = false: the step expected to end the solve, without the
// update that would orthonormalise its vector
static void right_step_one_gpu(Ctx &c, int j, const double *const *vp, double *z, double *w, bool update) {
    const bool direct = right_direct_output(c);
    const std::vector<const double *> dotp = dot_operands(vp, j, w);
    {
        DirectOutput out(c, direct, z);
        fieldsplit_apply(c, *c.amg, vp[j], z, 1.0, !direct);
    }
    product_and_dots(c, z, w, dotp.data(), j + 2, true);
    if (update) krylov_vector_update(c, j + 1, vp, w);
}

// One GPU, field split on the right, a step whose first Gram-Schmidt pass is expected to cancel (Ctx::KrylovHint): the
// step with its update, then the second pass in the queue (launch_cgs_refine) -- the first finish writes the flag the
// three kernels of the second pass read and leaves the step's one publication to them.  The fused product and the
// fused update must apply (three equations, j < 4, the producers forming the preconditioner's first stage).
static bool refined_step_applies(const Ctx &c, int j) {
    return !c.comm && c.iter_graphs_ok && !(c.prof.on && c.prof.all_kinds) && c.fs_first_by_producer &&
           !fieldsplit_upper(c) && spmv_dots_applicable(c, j + 2) && cgs_refine_applicable(c, j);
}

static bool iter_graph_launch_right_refined(Ctx &c, int j, const double *const *vp, double *z, double *w) {
    if (!refined_step_applies(c, j)) return false;
    return replay(c, c.iter_graph_refined, j, 1, [&] {
        const bool direct = right_direct_output(c);
        const std::vector<const double *> dotp = dot_operands(vp, j, w);
        {
            DirectOutput out(c, direct, z);
            fieldsplit_apply(c, *c.amg, vp[j], z, 1.0, !direct);
        }
        launch_spmv_dots(c, z, w, dotp.data(), j + 2, SPMV_DOTS_REFINED);
        krylov_vector_update(c, j + 1, vp, w);
        launch_cgs_refine(c, j, vp, w, reinterpret_cast<float *>(c.d_fs_g), c.amg->levels[0].b);
    });
}

// One GPU, field split on the right: Krylov steps j and j + 1 as ONE graph (a step needs nothing from the host, and
// when the previous solve says that both will be needed they are launched together anyway; between two graph
// launches the GPU idles for 8 us, tools/step_sequence.py).  Publishes twice: mail_seq advances by two.
static bool iter_graph_launch_right_pair(Ctx &c, int j, const double *const *vp, double *z0, double *w0, double *z1,
                                         double *w1, bool skip_last_update) {
    if (!switches().pairs || c.comm || !c.iter_graphs_ok || (c.prof.on && c.prof.all_kinds) || fieldsplit_upper(c))
        return false;
    return replay(c, skip_last_update ? c.iter_graph_pair_last : c.iter_graph_pair, j, 2, [&] {
        right_step_one_gpu(c, j, vp, z0, w0, true);
        right_step_one_gpu(c, j + 1, vp, z1, w1, !skip_last_update);
    });
}

static bool iter_graph_launch_right(Ctx &c, int j, const double *const *vp, double *z, double *w,
                                    bool skip_update = false) {
    if (!c.iter_graphs_ok || (c.prof.on && c.prof.all_kinds)) return false;
    const bool multi = c.comm != nullptr;
    if (skip_update && !multi)   // one GPU: the step expected to end the solve, without its update
        return replay(c, c.iter_graph_last, j, 1, [&] { right_step_one_gpu(c, j, vp, z, w, false); });
    if ((int)c.iter_graph.size() <= j) {
        c.iter_graph.resize(j + 1, nullptr);
        c.iter_graph_interior.resize(j + 1, nullptr);
        c.iter_graph_pre.resize(j + 1, nullptr);
    }
    if (!multi) return replay(c, c.iter_graph, j, 1, [&] { right_step_one_gpu(c, j, vp, z, w, true); });
    const bool upper = fieldsplit_upper(c);
    const bool direct = right_direct_output(c);
    const bool deep = deep_halo_active(c);
    // the cycle's leg up (deep halos) or the whole cycle, with its collectives, into z
    auto cycle_into_z = [&](bool leg_up_only) {
        {
            DirectOutput out(c, direct, z);
            if (leg_up_only) c.amg->vcycle(c, 0, 2);
            else c.amg->run(c);
        }
        if (!direct) fieldsplit_scatter(c, *c.amg, z);
    };
    if (!c.iter_graph[j]) {
        const std::vector<const double *> dotp = dot_operands(vp, j, w);
        bool ok = true;
        if (deep && !upper) {
            // deep halos: nothing is exchanged inside the step, so it is cut at its two all-reduces only --
            // [field split + the cycle's leg down] | level-1 all-reduce | [the cycle's leg up + the whole
            // Krylov product + local dot products] | all-reduce
            ok = capture_graph(c, &c.iter_graph_pre[j], [&] {
                {
                    DirectOutput out(c, direct, z);
                    fieldsplit_apply(c, *c.amg, vp[j], z, 1.0, !direct, false);
                }
                c.amg->vcycle(c, 0, 1);
            });
            ok = ok && capture_graph(c, &c.iter_graph[j], [&] {
                cycle_into_z(true);
                product_and_dots(c, z, w, dotp.data(), j + 2, false);
            });
        } else {
            Comm &cm = *c.comm;
            const bool cycle_inside = !c.amg->global;  // no collectives in the V-cycle
            ok = capture_graph(c, &c.iter_graph_pre[j], [&] {
                if (upper) {  // the V-cycle and its halo come before
                    fieldsplit_upper_species(c, *c.amg, vp[j], z, 1.0);
                } else {
                    DirectOutput out(c, direct, z);
                    fieldsplit_apply(c, *c.amg, vp[j], z, 1.0, !direct, cycle_inside);
                }
            });
            if (cm.n_interior)
                ok = ok && capture_graph(c, &c.iter_graph_interior[j], [&] {
                    launch_spmv(c, z, w, false, cm.d_interior, cm.n_interior);
                });
            ok = ok && capture_graph(c, &c.iter_graph[j], [&] {
                launch_spmv(c, z, w, false, cm.d_boundary, cm.n_boundary);
                launch_dots_fused(c, dotp.data(), w, j + 2, nullptr, false);
            });
        }
        if (!ok) {
            c.iter_graphs_ok = false;
            return false;
        }
    }
    // deep halos: v_j on all ghost layers, then sweeps, smoothings and the product without an exchange
    if (deep) comm_halo(c, const_cast<double *>(vp[j]));
    if (deep && !upper) {
        if (!launch_graph(c, c.iter_graph_pre[j])) {
            right_step_plain(c, j, vp, z, w, true);
            return true;
        }
        c.amg->allreduce_level1(c);
        if (!launch_graph(c, c.iter_graph[j])) {   // the same leg up and product, plainly
            cycle_into_z(true);
            plain_product_and_update(c, j, vp, z, w);
            return true;
        }
        reduce_and_update(c, j, vp, w);
        return true;
    }
    if (upper) {
        // potential first (the V-cycle with its collectives, then the ghost entries of its result), then the
        // species part: its graph, or plain launches -- with the exchanges between the sweeps, or because the
        // graph failed (same result)
        fieldsplit_upper_potential(c, *c.amg, vp[j], 1.0);
        if (c.fs_halo || !launch_graph(c, c.iter_graph_pre[j])) fieldsplit_upper_species(c, *c.amg, vp[j], z, 1.0);
    } else if (c.fs_halo && !deep) {
        // exchanges between the sweeps: the rank-local part of the preconditioner is not one graph
        DirectOutput out(c, direct, z);
        fieldsplit_apply(c, *c.amg, vp[j], z, 1.0, !direct, !c.amg->global);
    } else if (!launch_graph(c, c.iter_graph_pre[j])) {
        return false;  // nothing has been communicated yet: the caller repeats the step plainly
    }
    if (!upper && c.amg->global) cycle_into_z(false);  // V-cycle with its collectives
    const bool overlap = switches().halo_overlap;
    if (!deep && overlap) comm_halo_begin(c);   // (deep halos: z_j is exact on the first ghost layer already)
    else if (!deep) comm_halo(c, z);
    bool ok = !c.iter_graph_interior[j] || launch_graph(c, c.iter_graph_interior[j]);
    if (overlap && !deep) comm_halo_exchange(c, z);
    ok = ok && launch_graph(c, c.iter_graph[j]);
    if (!ok) {  // z_j is complete on every rank: redo the product with plain launches (same result)
        plain_product_and_update(c, j, vp, z, w);
        return true;
    }
    reduce_and_update(c, j, vp, w);
    return true;
}

// ---- GMRES(m) ---------------------------------------------------------------------------------
// Preconditioner on the left (point-block Jacobi; field split across GPUs): solves
// Minv J delta = Minv rhs (rhs in c.d_rhs, already scaled), convergence on the preconditioned
// residual norm |r| <= max(rtol*|r0|, atol).  (With fedm_set_krylov_scaling "rows" every norm below -- the right-hand
// side's, the recurrence's, the true residual's at the start of a cycle and in the reports -- is |D .|.)  Field split (one GPU by default, several always): on the right, flexible
// (z_j = Minv v_j kept, delta = Z y): rhs is -F itself, one preconditioner application less per
// solve, and the norm tested is that of the true residual.  delta starts at 0; classical
// Gram-Schmidt (PETSc's KSPGMRES default).
int gmres(Ctx &c, int restart, double rtol, double atol, int max_it, int *its_out, double *rnorm_out,
          const double *bvec, double bscale, double bnorm_known, double *u_update, bool *u_updated,
          int newton_iteration) {
    if (restart < 1 || restart > RED_K - 10) {
        set_error("GMRES restart must be between 1 and 30");
        return -2;
    }
    if (ensure_krylov(c, restart)) return -1;
    const int m = restart;
    HessenbergLeastSquares ls(m);
    std::vector<double> hcol(m + 1);
    std::vector<const double *> vp(m + 1), zp(m);
    for (int i = 0; i <= m; ++i) vp[i] = c.d_V + (size_t)i * c.np;
    for (int i = 0; i < m; ++i) zp[i] = c.d_Z + (size_t)i * c.np;
    const bool right = right_preconditioned(c);
    const bool fs_left = !right && c.amg && c.poisson;   // field split on the left (one GPU): the right-hand side is -M^-1 F
    // Row-equilibrated test (fedm_set_krylov_scaling): the same vectors, product and preconditioner, GMRES in the inner
    // product <x, y> = sum_i d_i^2 x_i y_i -- the iterates of GMRES on D J M^-1 D^-1 with the basis D^-1 V, so M^-1
    // receives D^-1 times a unit vector, not a scaled one.  Only the reductions change: for the duration of this solve
    // every launch_dots / launch_dots_fused / launch_spmv_dots / launch_norm2 takes the weights c.red_w.  Defined for
    // the field split on the right; on the left the tested residual M^-1 r is equilibrated already.
    const bool scaled = c.krylov_scaling != 0;
    if (scaled && !right) {
        set_error("krylov scaling 'rows' is defined for the field-split preconditioner on the right only (this solve "
                  "runs point-block Jacobi or the field split on the left): set the krylov scaling to 'none'");
        return -2;
    }
    struct ProducerMode {
        Ctx &c;
        ~ProducerMode() {
            c.fs_first_by_producer = false;
            c.red_w = nullptr;
        }
    } producer_mode{c};
    // one GPU, species sweeps, lower-triangular order: the producers of the Krylov vectors form the preconditioner's
    // first stage (krylov_vector_update); for the duration of this solve
    c.fs_first_by_producer = switches().first_by_producer && right && !c.comm && !fieldsplit_upper(c) &&
                             c.fs_sweeps > 1 && c.d_fs_g != nullptr;
    // the (unpreconditioned) operator of the right-preconditioned variant
    auto plain_operator = [&](double *v, double *w) {
        comm_halo(c, v);  // ghost inputs from their owners (multi-GPU)
        prof_begin(c, 1);
        launch_spmv(c, v, w, false);
        prof_end(c);
    };
    // The system is  J delta = bscale * bvec  (bvec = c.d_rhs, already preconditioned, on the left;
    // bvec = F, bscale = -1 on the right, where |bvec| is the |F| the Newton loop has just read:
    // bnorm_known >= 0).  u_update != nullptr: when the solve converges within its first cycle the
    // Newton update u += delta and the norms |delta|^2, |u|^2 (slots 1, 2) are formed by the kernel
    // that forms delta (*u_updated = true); c.d_delta is zeroed only if a generic update needs it.
    bool delta_zeroed = false;
    auto zero_delta = [&] {
        if (!delta_zeroed) hipMemsetAsync(c.d_delta, 0, sizeof(double) * c.np, c.stream);
        delta_zeroed = true;
    };
    if (u_updated) *u_updated = false;
    int64_t *ps = c.path_stats;
    ++ps[PS_SOLVES];
    // what the last solve of this kind took (Ctx::KrylovHint); a slot without history: what the previous solve took
    Ctx::KrylovHint &hint = c.krylov_hints[newton_iteration < 0 ? Ctx::KRYLOV_HINT_SLOTS
                                                                : std::min(newton_iteration, Ctx::KRYLOV_HINT_SLOTS - 1)];
    const int steps_hint = hint.its >= 0 ? hint.its : c.krylov_steps_hint;
    if (scaled) {
        // the weights of the Jacobian as it stands, and |D b|: the norm the caller knows is the unscaled one
        launch_row_scale(c, c.d_kscale2, nullptr);
        c.red_w = c.d_kscale2;
        launch_norm2(c, bvec, 0);
        read_red(c, 1);
        bnorm_known = std::sqrt(c.h_red[0]);
        if (!std::isfinite(bnorm_known)) {
            *its_out = 0;
            *rnorm_out = bnorm_known;
            return FEDM_DIVERGED_NAN;
        }
    }
    if (bnorm_known < 0.0) ++ps[PS_DEFERRED_NORM];
    int its = 0, cycle = 0;
    double r0 = -1.0, rnorm = 0.0;
    bool first = true;
    // The norm tested inside a cycle is the recurrence's |g[j+1]|; with ONE Gram-Schmidt pass it drifts from the true
    // residual as the basis loses orthogonality (measured: 5x below it after 11 steps at ksp_rtol 1e-7).  A solve
    // with the field split (either side) that ends on the generic update -- more than 8 steps, or a later cycle --
    // therefore goes round once more: the loop's top forms the true residual, reports it, and runs another cycle
    // if it is above the tolerance after all.  Given up (FEDM_DIVERGED_LINEAR with the true norm) when such a cycle
    // has not halved the true residual: the floor of the arithmetic is above the tolerance asked for.  Short solves
    // (the fused update) are left as they were; tests/test_gpu_krylov.py holds them to the same conditions.
    bool verifying = false;
    double verified_prev = -1.0;
    while (true) {
        // r = rhs - A delta  (delta == 0 on the first cycle)
        double *v0 = c.d_V;
        // (vector copies are kernels of ours: the runtime's blit copy runs at a tenth of the
        // memory bandwidth for these sizes)
        if (!first && fs_left) {
            // field split on the left: M^-1 (b - J delta) with b - J delta formed in double precision (b = -F), not
            // M^-1 b - M^-1 J delta: M^-1 rounds to single precision inside, and the difference of two vectors so
            // rounded says nothing below ~1e-7 |M^-1 b| (measured: code 0 with this residual at 4008x a 1e-10 tolerance)
            plain_operator(c.d_delta, c.d_w);
            launch_scale_copy(c, -1.0, c.d_w, c.d_w);
            launch_axpy(c, -1.0, c.d_F, c.d_w);
            fieldsplit_apply(c, *c.amg, c.d_w, v0, 1.0);
        } else if (!first) {
            if (right) plain_operator(c.d_delta, c.d_w);
            else apply_operator(c, c.d_delta, c.d_w);
            launch_scale_copy(c, bscale, bvec, v0);
            launch_axpy(c, -1.0, c.d_w, v0);
        }
        // First cycle: |rhs| is not waited for -- v0 is normalised on the device and the norm
        // rides along with the first Krylov step's publication (slot RED_SPARE).
        const bool deferred = first && bnorm_known < 0.0;
        double beta = 0.0, tol = 0.0;
        if (first && !deferred) {
            beta = bnorm_known;
            r0 = rnorm = beta;
            tol = std::max(rtol * r0, atol);
            first = false;
            if (beta <= tol) {  // nothing to solve
                ++ps[PS_NOTHING_TO_SOLVE];
                zero_delta();
                break;
            }
            krylov_vector_scale(c, bscale / beta, bvec, v0);
        } else if (deferred) {
            launch_norm2(c, bvec, RED_SPARE);
            launch_normalise_copy(c, RED_SPARE, bvec, v0);  // v0 = b / |b|  (bscale is 1 on this path)
            if (c.fs_first_by_producer) fieldsplit_first_stage(c, *c.amg, v0);
            first = false;
        } else {
            launch_norm2(c, v0, 0);
            read_red(c, 1);
            beta = std::sqrt(c.h_red[0]);
            if (!std::isfinite(beta)) {
                *its_out = its;
                *rnorm_out = beta;
                return FEDM_DIVERGED_NAN;
            }
            rnorm = beta;
            tol = std::max(rtol * r0, atol);
            ++ps[PS_VERIFIED];   // the true residual decides here, at the start of every cycle but the first
            if (verifying) {
                verifying = false;
                if (beta > tol) {
                    ++ps[PS_VERIFY_FAILED];
                    if (verified_prev >= 0.0 && beta > 0.5 * verified_prev) break;   // no progress: report it as it is
                    verified_prev = beta;
                }
            }
            if (beta > tol && its >= max_it) ++ps[PS_EXHAUSTED];
            if (beta <= tol || its >= max_it) break;
            krylov_vector_scale(c, 1.0 / beta, v0, v0);
        }
        ls.reset(beta);
        int j = 0;
        bool done = false;
        std::deque<unsigned long long> queued;
        int update_skipped_for = -1;   // step whose vector has not been orthonormalised yet (launched as 'the last one')
        uint32_t refined_launched = 0;   // bit q: step q went in with its second Gram-Schmidt pass behind it
        for (; j < m && its < max_it; ++j) {
            double *w = c.d_V + (size_t)(j + 1) * c.np;
            // classical Gram-Schmidt with ONE reduction and ONE host wait per iteration:
            // h_i = v_i.w and ww = w.w together; |w - V h|^2 = ww - |h|^2 on the device;
            // the update and the normalisation read their coefficients from device memory.
            auto launch_step = [&](int jj, bool skip_update = false) {
                double *ww = c.d_V + (size_t)(jj + 1) * c.np;
                if (right) {
                    double *z = c.d_Z + (size_t)jj * c.np;
                    if (skip_update && iter_graph_launch_right(c, jj, vp.data(), z, ww, true)) {
                        update_skipped_for = jj;
                        ++ps[PS_STEPS_LAST];
                        return c.mail_seq;
                    } else if (!iter_graph_launch_right(c, jj, vp.data(), z, ww)) {
                        right_step_plain(c, jj, vp.data(), z, ww, false);
                    }
                    ++ps[PS_STEPS_SINGLE];
                    return c.mail_seq;
                }
                ++ps[PS_STEPS_SINGLE];
                if (!iter_graph_launch(c, jj, vp.data(), ww)) {
                    apply_operator(c, vp[jj], ww);
                    launch_dots(c, dot_operands(vp.data(), jj, ww).data(), ww, jj + 2, true);
                    krylov_vector_update(c, jj + 1, vp.data(), ww);
                }
                return c.mail_seq;  // the sequence number of this step's publication
            };
            // A Krylov step needs nothing from the host (coefficients and normalisation stay on the
            // device), so the next one can be queued before this one's numbers arrive: the GPU does
            // not idle through the host's round trip and graph launch.  Done while the previous solve
            // says that step will be needed (one GPU: no collectives in between); a step launched in
            // vain only writes vectors nobody reads.
            // `queued`: publications of the steps j, j + 1, ... that are in the queue already.  Two steps go in as one
            // graph whenever two are wanted (between two graph launches the GPU idles for 8 us); a new pair is
            // launched when the queue has run empty, BEFORE this step's numbers are waited for -- so up to three
            // publications may be unread (MAIL_SLOTS).
            auto wanted = [&](int q) {   // step q is expected to be needed: launch it without waiting for step q - 1
                return right && !c.comm && q < m && its + (q - j) < max_it && q < steps_hint;
            };
            // The step expected to end the solve (the previous solve's count; early in a run: the second one) goes in
            // WITHOUT the update that would orthonormalise its vector for a next step: 8 us of kernel nobody needs when
            // the guess is right; when it is wrong the update is launched by itself before the solve goes on.
            auto ends_here = [&](int q) {
                return switches().skip_last_update && right && !c.comm && steps_hint >= 1 && steps_hint <= 4 &&
                       q + 1 == steps_hint && cycle == 0;
            };
            // The last solve of this kind needed a second Gram-Schmidt pass at step q: the step goes in by itself with
            // that pass queued behind it (never 'as the last one': the pass works on the updated vector)
            auto refine_predicted = [&](int q) {
                return right && cycle == 0 && q < 32 && ((hint.refine_mask >> q) & 1u) && refined_step_applies(c, q);
            };
            auto launch_from = [&](int q, bool first_is_needed) {
                if (q > 0 && update_skipped_for == q - 1 && (first_is_needed || wanted(q))) {   // (the guess was wrong)
                    krylov_vector_update(c, q, vp.data(), c.d_V + (size_t)q * c.np);
                    update_skipped_for = -1;
                    ++ps[PS_UPDATES_MADE_UP];
                }
                const size_t queued_before = queued.size();
                if ((first_is_needed || wanted(q)) && refine_predicted(q) &&
                    iter_graph_launch_right_refined(c, q, vp.data(), c.d_Z + (size_t)q * c.np,
                                                    c.d_V + (size_t)(q + 1) * c.np)) {
                    refined_launched |= 1u << q;
                    ++ps[PS_STEPS_SINGLE];
                    queued.push_back(c.mail_seq);
                } else if ((first_is_needed || wanted(q)) && wanted(q + 1) && !refine_predicted(q + 1) &&
                           iter_graph_launch_right_pair(c, q, vp.data(), c.d_Z + (size_t)q * c.np,
                                                        c.d_V + (size_t)(q + 1) * c.np, c.d_Z + (size_t)(q + 1) * c.np,
                                                        c.d_V + (size_t)(q + 2) * c.np, ends_here(q + 1))) {
                    if (ends_here(q + 1)) update_skipped_for = q + 1;
                    ps[PS_STEPS_PAIR] += ends_here(q + 1) ? 1 : 2;
                    ps[PS_STEPS_LAST] += ends_here(q + 1) ? 1 : 0;
                    queued.push_back(c.mail_seq - 1);
                    queued.push_back(c.mail_seq);
                } else if (first_is_needed || wanted(q)) {
                    queued.push_back(launch_step(q, ends_here(q)));
                }
                const int64_t ahead = (int64_t)(queued.size() - queued_before) - (first_is_needed ? 1 : 0);
                if (ahead > 0) {
                    ps[PS_STEPS_AHEAD] += ahead;
                    if (cycle > 0) ps[PS_STEPS_AHEAD_LATER] += ahead;
                }
            };
            if (queued.empty()) launch_from(j, true);
            const unsigned long long seq_j = queued.front();
            queued.pop_front();
            if (queued.empty()) launch_from(j + 1, false);
            wait_red_seq(c, seq_j);  // published by the finish kernel: the host works while the update runs
            if (comm_failed(c)) {  // a lost peer is an error, not a NaN
                *its_out = its;
                *rnorm_out = rnorm;
                return -1;
            }
            if (deferred && j == 0) {
                beta = std::sqrt(c.h_red[RED_SPARE]);
                if (!std::isfinite(beta)) {
                    ps[PS_STEPS_DROPPED] += 1 + (int64_t)queued.size();
                    *its_out = its;
                    *rnorm_out = beta;
                    return FEDM_DIVERGED_NAN;
                }
                r0 = rnorm = beta;
                tol = std::max(rtol * r0, atol);
                ls.reset(beta);
                if (beta <= tol) {  // nothing to solve: delta = 0 (j == 0: no update below)
                    ++ps[PS_NOTHING_TO_SOLVE];
                    ps[PS_STEPS_DROPPED] += 1 + (int64_t)queued.size();   // the step the norm rode on, too
                    zero_delta();
                    break;
                }
            }
            for (int i = 0; i <= j; ++i) hcol[i] = c.h_red[i];
            double hn2 = c.h_red[j + 1];
            const double ww = c.h_red[RED_K - 2];
            double hn;
            // a refined step: 0 the first pass was sound after all, 1 the second pass ran behind it (hcol and hn2 are
            // the refined ones), 2 it ran and the norm still cancels: the host's pass below, on the vector it left
            const int refined = ((refined_launched >> j) & 1u) ? (int)c.h_red[RED_REFINE] : -1;
            if (refined >= 0) {
                refined_launched &= ~(1u << j);
                if (refined == 0) hint.refine_mask &= ~(1u << j);
            }
            if (refined == 1) {
                ++ps[PS_SECOND_PASSES];
                ++ps[PS_SECOND_PASSES_DEVICE];
                hn = std::sqrt(hn2);
            } else if ((refined == 2 || !(hn2 > 1e-8 * ww && hn2 > 0.0)) && std::isfinite(ww) && ww > 0.0) {
                // strong cancellation: w was left unscaled; refine (second CGS pass) and
                // take the norm explicitly (a step launched ahead used the unrefined vector: let it
                // finish, its results are dropped and the step is repeated)
                ++ps[PS_SECOND_PASSES];
                if (cycle == 0 && j < 32) hint.refine_mask |= 1u << j;   // the next solve of this kind refines in the queue
                if (!queued.empty()) {
                    wait_red_seq(c, queued.back());
                    ps[PS_STEPS_DROPPED] += (int64_t)queued.size();
                    queued.clear();
                    refined_launched = 0;
                    // a dropped step that went in 'as the last one' is launched again from scratch: its skipped
                    // update must not be made up for a second time behind the relaunch
                    if (update_skipped_for > j) update_skipped_for = -1;
                }
                if (update_skipped_for == j) {   // the first Gram-Schmidt pass has not been applied to w yet
                    krylov_vector_update(c, j + 1, vp.data(), w);
                    update_skipped_for = -1;
                    ++ps[PS_UPDATES_MADE_UP];
                }
                launch_dots(c, vp.data(), w, j + 1, false);
                read_red(c, j + 1);
                for (int i = 0; i <= j; ++i) hcol[i] += c.h_red[i];
                launch_multi_axpy(c, c.h_red, j + 1, vp.data(), w, -1.0);
                launch_norm2(c, w, 0);
                read_red(c, 1);
                hn = std::sqrt(c.h_red[0]);
                if (hn > 0.0 && std::isfinite(hn)) krylov_vector_scale(c, 1.0 / hn, w, w);
            } else {
                hn = std::sqrt(hn2);
            }
            if (!std::isfinite(hn)) {
                ps[PS_STEPS_DROPPED] += 1 + (int64_t)queued.size();
                *its_out = its;
                *rnorm_out = hn;
                return FEDM_DIVERGED_NAN;
            }
            ++its;
            rnorm = ls.add_column(j, hcol.data(), hn);
            if (rnorm <= tol || hn == 0.0) {
                if (hn == 0.0) ++ps[PS_BREAKDOWNS];
                ps[PS_STEPS_DROPPED] += (int64_t)queued.size();   // launched ahead in vain
                ++j;
                done = true;
                break;
            }
        }
        const int k = j;
        const double *yv = ls.solve(k);   // delta += V y (Z y on the right)
        if (k > 0) {
            ++ps[PS_CYCLES];
            if (u_update && done && cycle == 0 && k <= 8) {
                launch_newton_update(c, yv, k, right ? zp.data() : vp.data(), u_update, nullptr);
                *u_updated = true;
                ++ps[PS_FUSED_UPDATES];
            } else {
                ++ps[PS_GENERIC_UPDATES];
                zero_delta();
                launch_multi_axpy(c, yv, k, right ? zp.data() : vp.data(), c.d_delta, 1.0);
            }
        }
        ++cycle;
        // the recurrence says converged: look at the true residual (point-block Jacobi on the left is all double
        // precision and needs many cycles anyway: left as it was)
        if (done && k > 0 && (right || fs_left) && !(u_updated && *u_updated)) {
            verifying = true;
            continue;
        }
        if (done || its >= max_it) {
            if (!done) {  // recompute the true (preconditioned, on the left) residual for the report
                ++ps[PS_EXHAUSTED];
                if (right) plain_operator(c.d_delta, c.d_w);
                else apply_operator(c, c.d_delta, c.d_w);
                launch_axpy(c, -bscale, bvec, c.d_w);
                launch_norm2(c, c.d_w, 0);
                read_red(c, 1);
                rnorm = std::sqrt(c.h_red[0]);
            }
            break;
        }
    }
    c.krylov_steps_hint = its;
    hint.its = its;
    ps[PS_STEPS_USED] += its;
    *its_out = its;
    *rnorm_out = rnorm;
    const double tol = std::max(rtol * r0, atol);
    return rnorm <= tol ? 0 : FEDM_DIVERGED_LINEAR;
}

// z = M^-1 v on the species block: the Richardson sweeps z += w_k Duu^-1 (v - J_uu z) from z = 0 with the weights of
// fedm_set_fieldsplit (one sweep of weight 1 when none is installed: point-block Jacobi).  c.d_tmp is scratch.
static void species_precondition(Ctx &c, const double *v, double *z) {
    launch_species_sweep(c, c.fs_main_w[0], v, nullptr, z, true);
    for (int k = 1; k < c.fs_main_sweeps; ++k) {
        launch_block_product(c, 0, z, c.d_tmp);
        launch_species_sweep(c, c.fs_main_w[k], v, c.d_tmp, z, false);
    }
}

// Flexible GMRES(restart) on J_uu delta_u = -F_u (F in c.d_F with zeros on the potential entries; delta in c.d_delta,
// zeros there too).  Classical Gram-Schmidt, two passes.  The recurrence's norm ends a cycle; success is reported only
// for a true residual |F_u + J_uu delta_u| <= max(rtol |F_u|, atol), formed in double precision at the top of the
// next cycle.  A cycle entered on such a check that does not halve the true residual gives up.
int species_gmres(Ctx &c, int restart, double rtol, double atol, int max_it, double bnorm, int *its_out,
                         double *rnorm_out) {
    if (restart < 1 || restart > RED_K - 10) {
        set_error("GMRES restart must be between 1 and 30");
        return -2;
    }
    if (ensure_krylov(c, restart)) return -1;
    const int m = restart;
    HessenbergLeastSquares ls(m);
    std::vector<double> hcol(m + 1);
    std::vector<const double *> vp(m + 1), zp(m);
    for (int i = 0; i <= m; ++i) vp[i] = c.d_V + (size_t)i * c.np;
    for (int i = 0; i < m; ++i) zp[i] = c.d_Z + (size_t)i * c.np;
    hipMemsetAsync(c.d_delta, 0, sizeof(double) * c.np, c.stream);
    const double tol = std::max(rtol * bnorm, atol);
    int its = 0;
    double rnorm = bnorm, verified_prev = -1.0;
    *its_out = 0;
    *rnorm_out = bnorm;
    if (bnorm <= tol) return 0;
    bool first = true, checking = false;
    while (true) {
        double *v0 = c.d_V;
        double beta = bnorm;
        if (first) {
            launch_scale_copy(c, -1.0 / beta, c.d_F, v0);
            first = false;
        } else {
            launch_block_product(c, 0, c.d_delta, c.d_w);
            launch_scale_copy(c, -1.0, c.d_F, v0);
            launch_axpy(c, -1.0, c.d_w, v0);
            launch_norm2(c, v0, 0);
            read_red(c, 1);
            beta = std::sqrt(c.h_red[0]);
            rnorm = beta;
            if (!std::isfinite(beta)) {
                c.seg_stats[SG_KRYLOV_STEPS] += its;
                *its_out = its;
                *rnorm_out = beta;
                return FEDM_DIVERGED_NAN;
            }
            if (beta <= tol) break;
            if (checking) {
                checking = false;
                if (verified_prev >= 0.0 && beta > 0.5 * verified_prev) break;   // the arithmetic's floor is above tol
                verified_prev = beta;
            }
            if (its >= max_it) break;
            launch_scale_copy(c, 1.0 / beta, v0, v0);
        }
        ls.reset(beta);
        int j = 0;
        bool done = false;
        for (; j < m && its < max_it; ++j) {
            double *z = c.d_Z + (size_t)j * c.np, *w = c.d_V + (size_t)(j + 1) * c.np;
            species_precondition(c, vp[j], z);
            launch_block_product(c, 0, z, w);
            for (int i = 0; i <= j; ++i) hcol[i] = 0.0;
            for (int pass = 0; pass < 2; ++pass) {
                launch_dots(c, vp.data(), w, j + 1, false);
                read_red(c, j + 1);
                for (int i = 0; i <= j; ++i) hcol[i] += c.h_red[i];
                launch_multi_axpy(c, c.h_red, j + 1, vp.data(), w, -1.0);
            }
            launch_norm2(c, w, 0);
            read_red(c, 1);
            const double hn = std::sqrt(c.h_red[0]);
            if (!std::isfinite(hn)) {
                c.seg_stats[SG_KRYLOV_STEPS] += its + 1;
                *its_out = its;
                *rnorm_out = hn;
                return FEDM_DIVERGED_NAN;
            }
            if (hn > 0.0) launch_scale_copy(c, 1.0 / hn, w, w);
            ++its;
            rnorm = ls.add_column(j, hcol.data(), hn);
            if (rnorm <= tol || hn == 0.0) {
                ++j;
                done = true;
                break;
            }
        }
        const int k = j;
        const double *yv = ls.solve(k);
        if (k > 0) launch_multi_axpy(c, yv, k, zp.data(), c.d_delta, 1.0);
        checking = done;   // the recurrence says converged: the loop's top looks at the true residual
    }
    c.seg_stats[SG_KRYLOV_STEPS] += its;
    *its_out = its;
    *rnorm_out = rnorm;
    return rnorm <= tol ? 0 : FEDM_DIVERGED_LINEAR;
}

// Jacobi- or multigrid-preconditioned CG (solver.hpp), shared by fedm_poisson_solve and fedm_poisson_update.  Every
// vector is zero on the species, Dirichlet and padding entries, so the iteration runs on the symmetric positive
// definite remainder.
CgResult preconditioned_cg(Ctx &c, CgMatrix matrix, double rtol, int max_it) {
    double *r = c.d_rhs, *z = c.d_tmp, *p = c.d_delta, *q = c.d_w, *x = c.d_V;
    auto precondition = [&] {
        if (c.amg) poisson_precondition(c, *c.amg, r, z);
        else if (matrix == CgMatrix::whole) launch_apply_dinv(c, r, z, 1.0);
        else launch_potential_jacobi(c, r, z);
    };
    // x = 0 (correction), z = Minv r, p = z
    precondition();
    launch_scale_copy(c, 1.0, z, p);
    const double *rz_ptr[1] = {r}, *pp[1] = {p};
    launch_dots(c, rz_ptr, z, 1);
    launch_norm2(c, r, 1);
    read_red(c, 2);
    double rz = c.h_red[0];
    const double r0 = std::sqrt(c.h_red[1]);
    double rn = r0;
    int it = 0;
    hipMemsetAsync(x, 0, sizeof(double) * c.np, c.stream);
    while (std::isfinite(rn) && rn > rtol * r0 && it < max_it) {
        if (matrix == CgMatrix::whole) {
            comm_halo(c, p);
            launch_spmv(c, p, q, false);
        } else {
            launch_block_product(c, 1, p, q);
        }
        launch_dots(c, pp, q, 1);
        read_red(c, 1);
        const double alpha = rz / c.h_red[0];
        launch_axpy(c, alpha, p, x);
        launch_axpy(c, -alpha, q, r);
        precondition();
        launch_dots(c, rz_ptr, z, 1);
        launch_norm2(c, r, 1);
        read_red(c, 2);
        const double rz_new = c.h_red[0];
        rn = std::sqrt(c.h_red[1]);
        if (!std::isfinite(rn)) break;
        const double beta = rz_new / rz;
        rz = rz_new;
        // p = z + beta p
        launch_scale_copy(c, beta, p, p);
        launch_axpy(c, 1.0, z, p);
        ++it;
    }
    return CgResult{it, r0, rn};
}

}  // namespace fedm
