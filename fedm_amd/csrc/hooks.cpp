// C ABI of libfedm_hip.so (include/fedm_hip.h): what tests, tools and the benchmark look through -- debug entry
// points, timers, counters, the profile -- and the installation of a transport.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "solver.hpp"

using namespace fedm;

extern "C" {

int fedm_debug_species_linear_solve(fedm_ctx *h, const double *b, const fedm_newton_opts *o, double *x, int *its,
                                    double *rnorm) {
    if (!h || !b || !o || !x) {
        set_error("fedm_debug_species_linear_solve: null argument");
        return -2;
    }
    Ctx &c = h->c;
    if (const int refused = segregated_refusal(c, "fedm_debug_species_linear_solve", true)) return refused;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (ensure_seg_dinv(c)) return -1;
    FEDM_HIP_CHECK(hipMemsetAsync(c.d_w, 0, sizeof(double) * c.np, c.stream));
    if (put_vec(c, c.d_w, b)) return -1;
    launch_pick_entries(c, 0, -1.0, c.d_w, c.d_F);   // species_gmres solves J_uu delta = -F
    launch_norm2(c, c.d_F, 0);
    read_red(c, 1);
    const double bnorm = std::sqrt(c.h_red[0]);
    int lits = 0;
    double lres = bnorm;
    int rc = FEDM_DIVERGED_NAN;
    if (std::isfinite(bnorm)) {
        launch_species_block_inverse(c);
        rc = species_gmres(c, o->ksp_restart, o->ksp_rtol, o->ksp_atol, o->ksp_max_it, bnorm, &lits, &lres);
    }
    if (its) *its = lits;
    if (rnorm) *rnorm = lres;
    if (rc < 0) return rc;
    if (get_vec(c, x, c.d_delta)) return -1;
    return rc;
}

int fedm_debug_species_assembly(fedm_ctx *h, int jacobian) {
    if (!h) {
        set_error("fedm_debug_species_assembly: null argument");
        return -2;
    }
    Ctx &c = h->c;
    if (const int refused = segregated_refusal(c, "fedm_debug_species_assembly", false)) return refused;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    const bool one_pass = launch_assemble_species(c, jacobian != 0);
    ++c.seg_stats[one_pass ? SG_ONE_PASS : SG_FALLBACK];
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipGetLastError());
    return one_pass ? 1 : 0;
}

int fedm_debug_block_product(fedm_ctx *h, int which, const double *x, double *y) {
    if (!h || !x || !y || (which != 0 && which != 1)) {
        set_error("fedm_debug_block_product: null argument, or a block other than 0 (species) and 1 (potential)");
        return -2;
    }
    Ctx &c = h->c;
    if (const int refused = segregated_refusal(c, "fedm_debug_block_product", false)) return refused;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipMemsetAsync(c.d_tmp, 0, sizeof(double) * c.np, c.stream));
    if (put_vec(c, c.d_tmp, x)) return -1;
    launch_block_product(c, which, c.d_tmp, c.d_w);
    return get_vec(c, y, c.d_w);
}

int fedm_debug_gd_reduced_field(fedm_ctx *h, double *out) {
    if (!h || !out) {
        set_error("fedm_debug_gd_reduced_field: null argument");
        return -2;
    }
    Ctx &c = h->c;
    if (c.model_kind != 1 || !c.gd_prep) {
        set_error("fedm_debug_gd_reduced_field: not an LMEA context, or fedm_gd_prep_setup has not been called");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    return gd_debug_reduced_field(c, out);
}

int fedm_debug_get_ext_source(fedm_ctx *h, int species, double *out) {
    if (!h || !out) {
        set_error("fedm_debug_get_ext_source: null argument");
        return -2;
    }
    Ctx &c = h->c;
    if (species < 0 || species >= c.ns || !c.d_ext[species]) {
        set_error("species has no Expression source");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipMemcpy(out, c.d_ext[species], sizeof(double) * (size_t)c.nc * c.model.ext_nodes[species],
                             hipMemcpyDeviceToHost));
    return 0;
}

int fedm_segregated_stats(fedm_ctx *h, int64_t out[8], int reset) {
    if (!h || (!out && !reset)) {
        set_error("fedm_segregated_stats: null argument");
        return -2;
    }
    Ctx &c = h->c;
    if (out)
        for (int i = 0; i < 8; ++i) out[i] = c.seg_stats[i];
    if (reset)
        for (int i = 0; i < 8; ++i) c.seg_stats[i] = 0;
    return 0;
}

int fedm_debug_species_planes_check(fedm_ctx *h, double *out) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (!out) {
        set_error("fedm_debug_species_planes_check: null argument");
        return -2;
    }
    return fieldsplit_planes_check(c, out, c.planes_last_fused);
}

int fedm_time_kernel(fedm_ctx *h, int kind, int repeats, double *ms_per_launch) {
    Ctx &c = h->c;
    if (kind == 6 && segregated_refusal(c, "fedm_time_kernel", false)) return -2;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    hipEvent_t e0, e1;
    FEDM_HIP_CHECK(hipEventCreate(&e0));
    FEDM_HIP_CHECK(hipEventCreate(&e1));
    auto run = [&]() {
        if (kind == 0) {
            launch_assemble(c, true, 0);
        } else if (kind == 1) {
            launch_spmv(c, c.d_u, c.d_w, false);
        } else if (kind == 3) {
            if (c.amg) c.amg->run(c);  // one multigrid cycle on the potential block (its replayed graph)
        } else if (kind == 4) {
            if (c.amg && c.poisson) fieldsplit_setup(c);   // the preconditioner's species planes from the assembled Jacobian
        } else if (kind == 5) {
            launch_assemble(c, true, 0);                   // ... behind the assembly, as in a Newton iteration
            c.boundary_pending = 0;
            if (c.amg && c.poisson) fieldsplit_setup(c);
        } else if (kind == 6) {
            launch_assemble_species(c, true, true);        // the volume kernel alone, as kind 0 times the coupled one
        } else {
            launch_assemble(c, false, 0);                  // (kinds 2 and 7: fedm_poisson_update's right-hand side is this assembly)
        }
    };
    run();  // warm-up
    c.boundary_pending = 0;   // (the volume kernel alone is timed: no launch_finalize follows)
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipEventRecord(e0, c.stream));
    for (int i = 0; i < repeats; ++i) run();
    FEDM_HIP_CHECK(hipEventRecord(e1, c.stream));
    FEDM_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    FEDM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_launch = (double)ms / repeats;
    c.boundary_pending = 0;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return 0;
}

int fedm_copy_bandwidth(int device, int64_t bytes, int repeats, double *gbs) {
    if (bytes < (1 << 20) || repeats < 1 || !gbs) {
        set_error("fedm_copy_bandwidth: at least 1 MiB and one repeat");
        return -2;
    }
    return copy_bandwidth(device, bytes, repeats, gbs);
}

// latency of the multi-GPU primitives on this context's transport, back to back on the compute
// stream: kind 0 = halo exchange of a block vector, 1 = of a scalar vector, 2 = all-reduce of 32
// doubles (what a Krylov step's dot products need)
int fedm_time_comm(fedm_ctx *h, int kind, int repeats, double *ms_per_op) {
    Ctx &c = h->c;
    if (!c.comm || kind < 0 || kind > 2 || repeats < 1 || !ms_per_op) {
        set_error("fedm_time_comm: no transport installed, or bad arguments");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    hipEvent_t e0, e1;
    FEDM_HIP_CHECK(hipEventCreate(&e0));
    FEDM_HIP_CHECK(hipEventCreate(&e1));
    auto run = [&]() {
        if (kind == 0) comm_halo(c, c.d_w);
        else if (kind == 1) comm_halo_scalar(c, c.d_w);
        else comm_allreduce(c, c.d_red, 32);
    };
    FEDM_HIP_CHECK(hipMemsetAsync(c.d_w, 0, sizeof(double) * c.np, c.stream));
    run();
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipEventRecord(e0, c.stream));
    for (int i = 0; i < repeats; ++i) run();
    FEDM_HIP_CHECK(hipEventRecord(e1, c.stream));
    FEDM_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    FEDM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_op = (double)ms / repeats;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (comm_failed(c)) {
        set_error(c.comm->error);
        return -1;
    }
    return 0;
}

int fedm_comm_unique_id(void *out128) { return comm_unique_id(out128); }

static int comm_common(Ctx &c, int n_nb, const int32_t *nb_rank, const int32_t *send_ptr,
                       const int32_t *send_idx, const int32_t *recv_ptr) {
    if (n_nb < 0 || (n_nb > 0 && (!nb_rank || !send_ptr || !recv_ptr))) {
        set_error("bad halo plan");
        return -2;
    }
    hipStreamSynchronize(c.stream);
    iter_graphs_clear(c);  // captured for the previous transport (or for none)
    if (c.comm) {
        c.comm->release();
        delete c.comm;
        c.comm = nullptr;
    }
    Comm *cm = new Comm();
    static const int32_t zero2[2] = {0, 0};
    const int rc = comm_setup_plan(c, *cm, n_nb, nb_rank, n_nb ? send_ptr : zero2, send_idx,
                                   n_nb ? recv_ptr : zero2);
    if (rc) {
        cm->release();
        delete cm;
        return rc;
    }
    c.comm = cm;
    return 0;
}

int fedm_comm_init_rccl(fedm_ctx *h, int n_nb, const int32_t *nb_rank, const int32_t *send_ptr,
                        const int32_t *send_idx, const int32_t *recv_ptr, const void *unique_id,
                        int rank, int n_ranks) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (int rc = comm_common(c, n_nb, nb_rank, send_ptr, send_idx, recv_ptr)) return rc;
    return comm_init_rccl(c, *c.comm, unique_id, rank, n_ranks);
}

int fedm_comm_init_callbacks(fedm_ctx *h, int n_nb, const int32_t *nb_rank, const int32_t *send_ptr,
                             const int32_t *send_idx, const int32_t *recv_ptr,
                             fedm_allreduce_fn allreduce, fedm_exchange_fn exchange, void *user,
                             int rank, int n_ranks) {
    Ctx &c = h->c;
    if (!allreduce || !exchange) {
        set_error("null transport callback");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (int rc = comm_common(c, n_nb, nb_rank, send_ptr, send_idx, recv_ptr)) return rc;
    c.comm->kind = 1;
    c.comm->rank = rank;
    c.comm->nranks = n_ranks;
    c.comm->allreduce_cb = allreduce;
    c.comm->exchange_cb = exchange;
    c.comm->user = user;
    return 0;
}

int fedm_comm_stats(fedm_ctx *h, int64_t out[10]) {
    Ctx &c = h->c;
    for (int i = 0; i < 10; ++i) out[i] = 0;
    if (!c.comm) return 0;
    const Comm &cm = *c.comm;
    out[0] = cm.kind;
    out[1] = cm.nranks;
    out[2] = cm.n_exchanges;
    out[3] = cm.n_allreduces;
    out[4] = cm.failed ? 1 : 0;
    out[5] = cm.n_nb;
    out[6] = cm.n_patch_interior;
    out[7] = cm.n_patch_boundary;
    out[8] = cm.halo_bytes;
    out[9] = cm.allreduce_bytes;
    return 0;
}

int fedm_debug_comm_fault(int fail_at, int64_t out[6]) { return comm_fault_selftest(fail_at, out); }

int fedm_debug_comm_roundtrip(fedm_ctx *h, double *vec, double *red, int k) {
    Ctx &c = h->c;
    if (!c.comm || !vec || k < 0 || k > RED_K || (k > 0 && !red)) {
        set_error("no transport on this context, or bad arguments");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipMemsetAsync(c.d_tmp, 0, sizeof(double) * c.np, c.stream));
    if (put_vec(c, c.d_tmp, vec)) return -1;
    comm_halo(c, c.d_tmp);          // on the compute stream ...
    comm_halo_begin(c);             // ... and once more the way the Krylov loop overlaps it: on the
    comm_halo_exchange(c, c.d_tmp); // communication stream, fenced by events (same values)
    if (k > 0) {
        FEDM_HIP_CHECK(hipMemcpyAsync(c.d_red, red, sizeof(double) * k, hipMemcpyHostToDevice, c.stream));
        comm_allreduce(c, c.d_red, k);
        comm_allreduce_f32_payload(c, c.d_red, k);   // the multigrid's single-precision payload (rounds to fp32)
        FEDM_HIP_CHECK(hipMemcpyAsync(red, c.d_red, sizeof(double) * k, hipMemcpyDeviceToHost, c.stream));
    }
    if (get_vec(c, vec, c.d_tmp)) return -1;
    if (comm_failed(c)) {
        set_error(c.comm->error);
        return -1;
    }
    return 0;
}

int fedm_debug_fieldsplit_tiles(fedm_ctx *h, int mode, int tile_slices, int depth, int threads) {
    if (!h) return -2;
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    iter_graphs_clear(c);   // captured Krylov steps hold the kernels of the old setting
    fs_tiles_configure(c, mode & 1, tile_slices, depth, threads);
    c.mg_tiles_off = (mode & 2) != 0;   // mode 3: species sweeps on tiles, the multigrid's finest-level sweeps not
    // the cycles' own graphs hold the kernels (and the tile tables) of the old setting: both hierarchies, the
    // one in use and the alternative for hard systems
    for (Amg *a : {c.amg, c.amg_alt})
        if (a && a->graph_exec) {
            hipGraphExecDestroy(a->graph_exec);
            a->graph_exec = nullptr;
        }
    return 0;
}

int fedm_debug_fieldsplit_apply(fedm_ctx *h, const double *t, double *z) {
    Ctx &c = h->c;
    if (!t || !z || !(c.amg && c.poisson)) {
        set_error("the field split needs a model with a Poisson row and a multigrid hierarchy (fedm_amg_setup)");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (put_vec(c, c.d_rhs, t)) return -1;
    fieldsplit_setup(c);
    fieldsplit_apply(c, *c.amg, c.d_rhs, c.d_w, 1.0);
    FEDM_HIP_CHECK(hipGetLastError());
    return get_vec(c, z, c.d_w);
}

int fedm_debug_fieldsplit_apply_operator(fedm_ctx *h, const double *v, double *t, double *z) {
    Ctx &c = h->c;
    if (!v || !t || !z || !(c.amg && c.poisson)) {
        set_error("the field split needs a model with a Poisson row and a multigrid hierarchy (fedm_amg_setup)");
        return -2;
    }
    if (fieldsplit_upper(c)) {
        set_error("fedm_debug_fieldsplit_apply_operator: the fused operator is the lower-triangular order's");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipMemsetAsync(c.d_rhs, 0, sizeof(double) * c.np, c.stream));   // (padding rows: as fedm_spmv)
    if (put_vec(c, c.d_rhs, v)) return -1;
    fieldsplit_setup(c);
    fieldsplit_apply_operator(c, *c.amg, c.d_rhs, c.d_tmp, c.d_w, true);
    FEDM_HIP_CHECK(hipGetLastError());
    if (get_vec(c, t, c.d_tmp)) return -1;
    return get_vec(c, z, c.d_w);
}

int fedm_debug_fieldsplit_apply_produced(fedm_ctx *h, const double *t, int k, const double *coef, double *y,
                                          double *z) {
    Ctx &c = h->c;
    if (!t || !coef || !y || !z || !(c.amg && c.poisson) || k < 0 || k > 8) {
        set_error("fedm_debug_fieldsplit_apply_produced: bad arguments, or no field split (fedm_amg_setup)");
        return -2;
    }
    // the condition under which gmres lets the producers form the first stage (FEDM_FS_FIRST_BY_PRODUCER), the
    // preconditioner's side aside
    if (c.comm || fieldsplit_upper(c) || c.fs_sweeps < 2 || !c.d_fs_g) {
        set_error("fedm_debug_fieldsplit_apply_produced: the producers form no first stage here (one GPU, lower-"
                  "triangular order, species sweeps)");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipMemsetAsync(c.d_rhs, 0, sizeof(double) * c.np, c.stream));
    FEDM_HIP_CHECK(hipMemsetAsync(c.d_tmp, 0, sizeof(double) * c.np, c.stream));
    if (put_vec(c, c.d_rhs, t)) return -1;
    fieldsplit_setup(c);
    c.fs_first_by_producer = true;
    if (k == 0) {
        krylov_vector_scale(c, coef[0], c.d_rhs, c.d_tmp);
    } else {
        // the Gram-Schmidt coefficients where gmres's reduction leaves them: h_i in d_red[i], 1/|.| in d_red[RED_K-1]
        std::vector<double> red(RED_K, 0.0);
        for (int i = 0; i < k; ++i) red[i] = coef[i];
        red[RED_K - 1] = coef[k];
        FEDM_HIP_CHECK(hipMemcpyAsync(c.d_red, red.data(), sizeof(double) * RED_K, hipMemcpyHostToDevice, c.stream));
        FEDM_HIP_CHECK(hipMemcpyAsync(c.d_tmp, c.d_rhs, sizeof(double) * c.np, hipMemcpyDeviceToDevice, c.stream));
        std::vector<const double *> vp((size_t)k, c.d_rhs);
        krylov_vector_update(c, k, vp.data(), c.d_tmp);
    }
    fieldsplit_apply(c, *c.amg, c.d_tmp, c.d_w, 1.0);
    c.fs_first_by_producer = false;
    FEDM_HIP_CHECK(hipGetLastError());
    if (get_vec(c, y, c.d_tmp)) return -1;
    return get_vec(c, z, c.d_w);
}

}  // extern "C"

// ---- fedm_debug_krylov_op: one launch wrapper of the Krylov step on the caller's vectors -----------------------------
namespace {

static_assert(FEDM_KOP_RED_K == RED_K, "fedm_krylov_io::red mirrors Ctx::d_red");

// a host vector into a device vector of c.np entries: the caller's first n_keep entries, the sentinel behind them
int put_with_sentinel(Ctx &c, double *dst, const double *src, size_t n_keep, double sentinel) {
    for (size_t i = 0; i < (size_t)c.np; ++i) c.h_stage[i] = sentinel;
    if (src) std::memcpy(c.h_stage, src, sizeof(double) * n_keep);
    FEDM_HIP_CHECK(hipMemcpyAsync(dst, c.h_stage, sizeof(double) * c.np, hipMemcpyHostToDevice, c.stream));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    return 0;
}

int krylov_op_refuse(const char *why) {
    set_error(std::string("fedm_debug_krylov_op: ") + why);
    return -2;
}

// what the op does to the context's own vectors is undone on every way out
struct KrylovOpGuard {
    Ctx &c;
    std::vector<double> red;
    bool state_saved = false, first_stage_written = false;
    KrylovOpGuard(Ctx &ctx, const std::vector<double> &red_as_found) : c(ctx), red(red_as_found) {}
    ~KrylovOpGuard() {
        c.red_w = nullptr;
        hipMemcpyAsync(c.d_red, red.data(), sizeof(double) * 2 * RED_K, hipMemcpyHostToDevice, c.stream);
        if (first_stage_written) {
            hipMemsetAsync(c.d_fs_g, 0, sizeof(double) * c.np, c.stream);
            hipMemsetAsync(c.amg->levels[0].b, 0, sizeof(double) * c.nvp, c.stream);
        }
        if (state_saved) {
            hipMemcpyAsync(c.d_u, c.d_Z + (size_t)c.np, sizeof(double) * c.np, hipMemcpyDeviceToDevice, c.stream);
            hipMemcpyAsync(c.d_uold, c.d_Z + 2 * (size_t)c.np, sizeof(double) * c.np, hipMemcpyDeviceToDevice, c.stream);
        }
        hipStreamSynchronize(c.stream);
    }
};

}  // namespace

extern "C" {

int fedm_debug_krylov_op(fedm_ctx *h, int op, int k, fedm_krylov_io *io) {
    if (!h || !io || !io->red) return krylov_op_refuse("null argument");
    Ctx &c = h->c;
    if (op < 0 || op >= FEDM_KOP_COUNT) return krylov_op_refuse("unknown op");
    if (!std::isfinite(io->sentinel)) return krylov_op_refuse("the sentinel must be finite");
    if (io->n_vec < 0 || io->n_vec > FEDM_KOP_MAX_VECTORS || (io->n_vec > 0 && !io->V))
        return krylov_op_refuse("n_vec out of range (0 .. 32), or no V");
    const bool fs_op = op == FEDM_KOP_CGS_UPDATE_FS || op == FEDM_KOP_SCALE_COPY_FS || op == FEDM_KOP_CGS_REFINE;
    const bool uses_V = op == FEDM_KOP_DOTS || op == FEDM_KOP_DOTS_FUSED || op == FEDM_KOP_SPMV_DOTS ||
                        op == FEDM_KOP_CGS_REFINE || op == FEDM_KOP_CGS_UPDATE || op == FEDM_KOP_CGS_UPDATE_FS ||
                        op == FEDM_KOP_MULTI_AXPY || op == FEDM_KOP_NEWTON_UPDATE;
    const bool uses_x = op == FEDM_KOP_SPMV_DOTS || op == FEDM_KOP_SCALE_COPY_FS || op == FEDM_KOP_NORMALISE_COPY ||
                        op == FEDM_KOP_FIELD_ERROR || op == FEDM_KOP_FIELD_ERROR_SLOTS34;
    const bool y_is_V = op == FEDM_KOP_DOTS_FUSED && io->y_index >= 0;
    const bool y_is_output_only = op == FEDM_KOP_SPMV_DOTS || op == FEDM_KOP_SCALE_COPY_FS ||
                                  op == FEDM_KOP_NORMALISE_COPY;
    // ---- arguments: every refusal comes before the first launch
    int n_basis = 0;   // the vectors of V the op reads
    switch (op) {
        case FEDM_KOP_DOTS:
        case FEDM_KOP_DOTS_FUSED:
        case FEDM_KOP_CGS_UPDATE:
        case FEDM_KOP_MULTI_AXPY:
            if (k < 1 || k > FEDM_KOP_MAX_VECTORS) return krylov_op_refuse("k out of range (1 .. 32)");
            n_basis = k;
            break;
        case FEDM_KOP_SPMV_DOTS:
            if (c.neq != 3) return krylov_op_refuse("the product fused with the dots exists for three equations only");
            if (k < 2 || k > 8) return krylov_op_refuse("k out of range (2 .. 8)");
            if (io->finish < 0 || io->finish > 2) return krylov_op_refuse("finish out of range (0 .. 2)");
            n_basis = k - 1;
            break;
        case FEDM_KOP_CGS_REFINE:
            if (k < 2 || k > 5) return krylov_op_refuse("k out of range (2 .. 5)");
            n_basis = k - 1;
            break;
        case FEDM_KOP_CGS_UPDATE_FS:
            if (k < 1 || k > 4) return krylov_op_refuse("k out of range (1 .. 4)");
            n_basis = k;
            break;
        case FEDM_KOP_NEWTON_UPDATE:
            if (k < 1 || k > 8) return krylov_op_refuse("k out of range (1 .. 8)");
            n_basis = k;
            break;
        case FEDM_KOP_NORM2_PUBLISH:
            if (k < 1 || k > RED_K) return krylov_op_refuse("k out of range (1 .. RED_K)");
            [[fallthrough]];
        case FEDM_KOP_NORM2:
        case FEDM_KOP_NORMALISE_COPY:
            if (io->slot < 0 || io->slot >= RED_K) return krylov_op_refuse("slot out of range");
            break;
        case FEDM_KOP_FIELD_ERROR:
        case FEDM_KOP_FIELD_ERROR_SLOTS34:
            if (io->slot < 0 || io->slot >= c.neq) return krylov_op_refuse("component out of range");
            break;
        default: break;
    }
    if (uses_V && n_basis > io->n_vec) return krylov_op_refuse("k beyond the vectors in V");
    if (y_is_V && io->y_index >= io->n_vec) return krylov_op_refuse("y_index beyond the vectors in V");
    if (!y_is_V && !y_is_output_only && !io->y) return krylov_op_refuse("no y");
    if (uses_x && !io->x) return krylov_op_refuse("no x");
    if ((op == FEDM_KOP_MULTI_AXPY || op == FEDM_KOP_NEWTON_UPDATE) && !io->coef) return krylov_op_refuse("no coef");
    if (fs_op && (c.ns != 2 || !(c.amg && c.poisson) || !c.d_fs_g || c.comm))
        return krylov_op_refuse("the fused first stage needs two species, one GPU and the field split's buffers "
                                "(fedm_amg_setup)");
    if (c.krylov_scaling != 0 && !c.d_kscale2) return krylov_op_refuse("krylov scaling without its weights");
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    // ---- storage, and the counters as found
    const double *V_before = c.d_V;
    if (ensure_krylov(c, 30)) return -1;   // (clears the captured steps itself when it reallocates)
    io->info[3] = c.d_V != V_before ? 1 : 0;
    unsigned long long dev_seq = 0;
    FEDM_HIP_CHECK(hipMemcpy(&dev_seq, c.d_mail_seq, sizeof(dev_seq), hipMemcpyDeviceToHost));
    if (dev_seq != c.mail_seq) {
        io->info[0] = io->info[2] = -1;
        io->info[1] = (int64_t)c.mail_seq;
        return krylov_op_refuse("the host's and the device's publication counts are apart");
    }
    const unsigned long long seq_before = c.mail_seq;
    std::vector<double> red_as_found(2 * RED_K);
    FEDM_HIP_CHECK(hipMemcpy(red_as_found.data(), c.d_red, sizeof(double) * 2 * RED_K, hipMemcpyDeviceToHost));
    KrylovOpGuard guard(c, red_as_found);
    // ---- the caller's vectors
    const size_t n_red = (size_t)c.n_dot;     // entries that take part in reductions: the owned rows
    auto V_at = [&](int i) { return i < 31 ? c.d_V + (size_t)i * c.np : c.d_Z; };
    std::vector<const double *> vp(FEDM_KOP_MAX_VECTORS, nullptr);
    for (int i = 0; i < io->n_vec; ++i) {
        vp[i] = V_at(i);
        if (put_with_sentinel(c, V_at(i), io->V + (size_t)i * c.n, n_red, io->sentinel)) return -1;
    }
    double *y = y_is_V ? V_at(io->y_index) : c.d_w;
    if (!y_is_V && put_with_sentinel(c, c.d_w, y_is_output_only ? nullptr : io->y, n_red, io->sentinel)) return -1;
    double *x = c.d_tmp;
    if (op == FEDM_KOP_DOTS_FUSED && io->x0) {
        if (put_with_sentinel(c, x, io->x0, (size_t)c.nv, io->sentinel)) return -1;
    } else {
        if (put_with_sentinel(c, x, uses_x ? io->x : nullptr, op == FEDM_KOP_SPMV_DOTS ? (size_t)c.n : n_red,
                              io->sentinel))
            return -1;
    }
    if (io->red_in)
        FEDM_HIP_CHECK(hipMemcpyAsync(c.d_red, io->red, sizeof(double) * 2 * RED_K, hipMemcpyHostToDevice, c.stream));
    else
        FEDM_HIP_CHECK(hipMemsetAsync(c.d_red, 0, sizeof(double) * 2 * RED_K, c.stream));
    float *g32 = reinterpret_cast<float *>(c.d_fs_g);
    double *b0 = fs_op ? c.amg->levels[0].b : nullptr;
    if (fs_op) {
        fieldsplit_setup(c);   // Duu^-1 of the Jacobian as it stands
        guard.first_stage_written = true;
        // (what the op does not write shows: g32 holds np doubles' worth of bytes, b0 the padded vertices)
        FEDM_HIP_CHECK(hipMemsetAsync(c.d_fs_g, 0xff, sizeof(double) * c.np, c.stream));
        FEDM_HIP_CHECK(hipMemsetAsync(b0, 0xff, sizeof(double) * c.nvp, c.stream));
    }
    if (c.krylov_scaling != 0) {
        launch_row_scale(c, c.d_kscale2, nullptr);
        c.red_w = c.d_kscale2;
    }
    // ---- the op
    bool launched = true;
    switch (op) {
        case FEDM_KOP_DOTS: launch_dots(c, vp.data(), y, k, io->finish != 0); break;
        case FEDM_KOP_DOTS_FUSED:
            launch_dots_fused(c, vp.data(), y, k, io->x0 ? x : nullptr, io->finish != 0);
            break;
        case FEDM_KOP_SPMV_DOTS: launched = launch_spmv_dots(c, x, y, vp.data(), k, io->finish); break;
        case FEDM_KOP_CGS_REFINE: launched = launch_cgs_refine(c, k - 2, vp.data(), y, g32, b0); break;
        case FEDM_KOP_NORM2: launch_norm2(c, y, io->slot); break;
        case FEDM_KOP_NORM2_PUBLISH: norm2_publish(c, y, io->slot, k); break;
        case FEDM_KOP_CGS_UPDATE: launch_cgs_update(c, k, vp.data(), y); break;
        case FEDM_KOP_CGS_UPDATE_FS: launched = launch_cgs_update_fs(c, k, vp.data(), y, g32, b0); break;
        case FEDM_KOP_SCALE_COPY_FS: launched = launch_scale_copy_fs(c, io->a, x, y, g32, b0); break;
        case FEDM_KOP_MULTI_AXPY: launch_multi_axpy(c, io->coef, k, vp.data(), y, io->a); break;
        case FEDM_KOP_NEWTON_UPDATE:
            launch_newton_update(c, io->coef, k, vp.data(), y, io->finish ? x : nullptr);
            break;
        case FEDM_KOP_NORMALISE_COPY: launch_normalise_copy(c, io->slot, x, y); break;
        default: {   // the field error reads the state itself: the caller's vectors stand in for it, the state comes back
            double *keep_u = c.d_Z + (size_t)c.np, *keep_old = c.d_Z + 2 * (size_t)c.np;
            FEDM_HIP_CHECK(hipMemcpyAsync(keep_u, c.d_u, sizeof(double) * c.np, hipMemcpyDeviceToDevice, c.stream));
            FEDM_HIP_CHECK(hipMemcpyAsync(keep_old, c.d_uold, sizeof(double) * c.np, hipMemcpyDeviceToDevice, c.stream));
            guard.state_saved = true;
            FEDM_HIP_CHECK(hipMemcpyAsync(c.d_u, y, sizeof(double) * c.np, hipMemcpyDeviceToDevice, c.stream));
            FEDM_HIP_CHECK(hipMemcpyAsync(c.d_uold, x, sizeof(double) * c.np, hipMemcpyDeviceToDevice, c.stream));
            if (op == FEDM_KOP_FIELD_ERROR) launch_field_error(c, io->slot);
            else launch_field_error_slots34(c, io->slot);
        }
    }
    c.red_w = nullptr;
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipGetLastError());
    if (!launched) {
        set_error("fedm_debug_krylov_op: the launch wrapper has no kernel for this case");
        return -2;
    }
    // ---- what it left
    FEDM_HIP_CHECK(hipMemcpy(io->red, c.d_red, sizeof(double) * 2 * RED_K, hipMemcpyDeviceToHost));
    FEDM_HIP_CHECK(hipMemcpy(&dev_seq, c.d_mail_seq, sizeof(dev_seq), hipMemcpyDeviceToHost));
    io->info[0] = (int64_t)(c.mail_seq - seq_before);
    io->info[1] = (int64_t)c.mail_seq;
    io->info[2] = (int64_t)dev_seq;
    if (io->info[0] > 0 && dev_seq == c.mail_seq) {
        wait_red(c);
        if (io->mail) std::memcpy(io->mail, c.h_red, sizeof(double) * RED_K);
    }
    if (io->y_out && get_vec(c, io->y_out, y)) return -1;
    if (io->x_out && get_vec(c, io->x_out, x)) return -1;
    if (fs_op && io->g32)
        FEDM_HIP_CHECK(hipMemcpy(io->g32, g32, sizeof(float) * (size_t)c.nv * 2, hipMemcpyDeviceToHost));
    if (fs_op && io->b0) FEDM_HIP_CHECK(hipMemcpy(io->b0, b0, sizeof(double) * c.nv, hipMemcpyDeviceToHost));
    if (dev_seq != c.mail_seq) {
        set_error("fedm_debug_krylov_op: the op left the host's and the device's publication counts apart");
        return -1;
    }
    return 0;
}

int fedm_pattern_stats(const fedm_mesh_desc *mesh, int64_t out[12]) {
    if (!mesh || !out || mesh->n_vertices < 3 || mesh->n_cells < 1) {
        set_error("null or empty mesh");
        return -2;
    }
    for (int i = 0; i < 3 * mesh->n_cells; ++i)
        if (mesh->cells[i] < 0 || mesh->cells[i] >= mesh->n_vertices) {
            set_error("cell vertex index out of range");
            return -2;
        }
    Pattern pat;
    build_pattern(*mesh, pat);
    // LDS-atomic clashes of the patch cell order: for each lane group of 16 cells and each local
    // vertex index a, owned a-vertices that fall into an accumulator bank class (id mod 16) another
    // cell of the group already uses
    int64_t pairs = 0, clashes = 0;
    for (int s = 0; s < pat.n_slices; ++s) {
        const int c0 = pat.patch_cell_ptr[s], c1 = pat.patch_cell_ptr[s + 1];
        for (int g0 = c0; g0 < c1; g0 += 16)
            for (int a = 0; a < 3; ++a) {
                uint32_t used = 0;
                for (int k = g0; k < std::min(g0 + 16, c1); ++k) {
                    const int lv = pat.patch_cells[k].lv[a];
                    if (lv >= SLICE) continue;
                    ++pairs;
                    if ((used >> (lv & 15)) & 1u) ++clashes;
                    used |= 1u << (lv & 15);
                }
            }
    }
    out[0] = pat.n_slices;
    out[1] = pat.max_patch_cells;
    out[2] = pat.max_patch_width;
    out[3] = pat.max_patch_verts;
    out[4] = (int64_t)pat.patch_cells.size();
    out[5] = pairs;
    out[6] = clashes;
    out[7] = pat.nnz_blocks;
    out[8] = pat.total_bc * SLICE;
    out[9] = (int64_t)pat.patch_halo.size();
    out[10] = (int64_t)pat.colour_ptr.size() - 1;
    // emission blocks: (wave of 64 cells, local row a) pairs in which some cell owns its a-th vertex -- the
    // assembly kernels skip the others (at most 3 per wave)
    int64_t blocks = 0;
    for (int s = 0; s < pat.n_slices; ++s) {
        const int c0 = pat.patch_cell_ptr[s], c1 = pat.patch_cell_ptr[s + 1];
        for (int w0 = c0; w0 < c1; w0 += SLICE)
            for (int a = 0; a < 3; ++a) {
                bool any = false;
                for (int k = w0; k < std::min(w0 + SLICE, c1); ++k) any = any || pat.patch_cells[k].lv[a] < SLICE;
                blocks += any;
            }
    }
    out[11] = blocks;
    return 0;
}

int fedm_profile(fedm_ctx *h, int enable) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    Prof &p = c.prof;
    prof_collect(c);
    if (enable && p.ev.empty()) {
        p.ev.resize(16384);
        p.kind.resize(8192);
        for (auto &e : p.ev) FEDM_HIP_CHECK(hipEventCreate(&e));
    }
    p.on = enable != 0;
    p.all_kinds = enable == 2;  // SpMV / V-cycle events need plain launches (no iteration graphs)
    if (enable)
        for (int k = 0; k < 8; ++k) {
            p.ms[k] = 0.0;
            p.cnt[k] = 0;
            p.seen[k] = 0;
        }
    return 0;
}

int fedm_profile_read(fedm_ctx *h, int kind, double *ms_total, int64_t *count) {
    Ctx &c = h->c;
    if (kind < 0 || kind >= 8) return -2;
    prof_collect(c);
    // kinds that are sampled (Prof::stride) report the sampled mean times the launches seen
    const Prof &p = c.prof;
    const double mean = p.cnt[kind] ? p.ms[kind] / (double)p.cnt[kind] : 0.0;
    if (ms_total) *ms_total = mean * (double)p.seen[kind];
    if (count) *count = p.seen[kind];
    return 0;
}

int fedm_launched_assembly(fedm_ctx *h, int64_t out[8]) {
    if (!h || !out) return -2;
    const Ctx &c = h->c;
    for (int j = 0; j < 2; ++j)
        for (int k = 0; k < 4; ++k) out[4 * j + k] = c.launched[j][k];
    return 0;
}

int fedm_solver_path_stats(fedm_ctx *h, int64_t out[24], int reset) {
    if (!h) return -2;
    Ctx &c = h->c;
    static_assert(PS_COUNT <= 24, "fedm_solver_path_stats reports 24 counters");
    if (out)
        for (int k = 0; k < 24; ++k) out[k] = c.path_stats[k];
    if (reset)
        for (int64_t &v : c.path_stats) v = 0;
    return 0;
}

// J x = b with the assembled Jacobian, through the call fedm_newton_solve makes (same preparation of the
// preconditioner and the right-hand side, same conventions for the side in use); the state is not touched.
// The right-hand side travels as F = -b, so the residual of the last assembly is overwritten.
int fedm_debug_linear_solve(fedm_ctx *h, const double *b, const fedm_newton_opts *o, double *x, int *its,
                            double *rnorm) {
    if (!h || !b || !o || !x) {
        set_error("fedm_debug_linear_solve: null argument");
        return -2;
    }
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (put_vec(c, c.d_rhs, b)) return -1;
    launch_scale_copy(c, -1.0, c.d_rhs, c.d_F);
    launch_norm2(c, c.d_F, 0);
    read_red(c, 1);
    const double fnorm = std::sqrt(c.h_red[0]);
    prepare_preconditioner_and_rhs(c);
    const bool right = right_preconditioned(c);
    int lits = 0;
    double lres = 0.0;
    const int rc = gmres(c, o->ksp_restart, o->ksp_rtol, o->ksp_atol, o->ksp_max_it, &lits, &lres,
                         right ? c.d_F : c.d_rhs, right ? -1.0 : 1.0, right ? fnorm : -1.0, nullptr, nullptr);
    if (its) *its = lits;
    if (rnorm) *rnorm = lres;
    if (rc < 0) return rc;
    if (get_vec(c, x, c.d_delta)) return -1;
    if (comm_failed(c)) {
        set_error(c.comm->error);
        return -1;
    }
    if (hipGetLastError() != hipSuccess) {
        set_error("HIP error during the linear solve");
        return -1;
    }
    return rc;
}

int fedm_fieldsplit_tiles_stats(const fedm_mesh_desc *mesh, int tile_slices, int depth, int64_t out[10]) {
    if (!mesh || !out || mesh->n_vertices < 3 || mesh->n_cells < 1) {
        set_error("null or empty mesh");
        return -2;
    }
    for (int i = 0; i < 3 * mesh->n_cells; ++i)
        if (mesh->cells[i] < 0 || mesh->cells[i] >= mesh->n_vertices) {
            set_error("cell vertex index out of range");
            return -2;
        }
    long long v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = fs_tiles_host_stats(*mesh, tile_slices, depth, v);
    if (rc) {
        set_error("tile parameters out of range (1..8 slices, 1..8 layers) or a tile too large for 16-bit local indices");
        return rc;
    }
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return 0;
}

int fedm_fieldsplit_tiles_info(fedm_ctx *h, int64_t out[10]) {
    if (!h || !out) return -2;
    long long v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int in_use = fs_tiles_info(h->c, v);
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return in_use;
}

int64_t fedm_block_nnz(fedm_ctx *h) { return h->c.pat.nnz_blocks; }

int fedm_block_csr(fedm_ctx *h, int cr, int cc, int64_t *indptr, int32_t *indices, double *values) {
    Ctx &c = h->c;
    if (cr < 0 || cr >= c.neq || cc < 0 || cc >= c.neq) {
        set_error("block component out of range");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    const int neq2 = c.neq * c.neq;
    const size_t nplane = (size_t)c.pat.total_bc * SLICE;
    std::vector<double> plane(nplane);
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    // one strided 2-D copy: plane e of every block column
    FEDM_HIP_CHECK(hipMemcpy2D(plane.data(), sizeof(double) * SLICE,
                               c.d_val + (size_t)(cr * c.neq + cc) * SLICE,
                               sizeof(double) * SLICE * neq2, sizeof(double) * SLICE,
                               (size_t)c.pat.total_bc, hipMemcpyDeviceToHost));
    int64_t pos = 0;
    indptr[0] = 0;
    for (int v = 0; v < c.nv; ++v) {
        const int s = v / SLICE, l = v % SLICE;
        for (int j = 0; j < c.pat.row_len[v]; ++j) {
            const size_t bc = (size_t)c.pat.slice_boff[s] + j;
            indices[pos] = c.pat.colidx[bc * SLICE + l];
            values[pos] = plane[bc * SLICE + l];
            ++pos;
        }
        indptr[v + 1] = pos;
    }
    return 0;
}

}  // extern "C"
