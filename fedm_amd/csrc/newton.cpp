// C ABI of libfedm_hip.so (include/fedm_hip.h): residual and Jacobian, the Newton loops, the Poisson solves.
// Host logic only; the linear solvers are in krylov.cpp.
#include <chrono>
#include <cmath>

#include "solver.hpp"

namespace fedm {

// the alternative set of species sweeps and (when installed) the alternative V-cycle, together
void set_hard_mode(Ctx &c, bool hard) {
    if (c.fs_alt_active == hard) return;
    c.fs_skip_sample = true;   // (measured policy: the next solve captures its graphs anew)
    hipStreamSynchronize(c.stream);
    iter_graphs_clear(c);  // the captured steps contain the other sweeps / the other cycle
    c.fs_alt_active = hard;
    if (c.fs_alt_sweeps > 0) {
        c.fs_sweeps = hard ? c.fs_alt_sweeps : c.fs_main_sweeps;
        for (int i = 0; i < c.fs_sweeps; ++i) c.fs_w[i] = hard ? c.fs_alt_w[i] : c.fs_main_w[i];
    }
    if (c.amg_alt) std::swap(c.amg, c.amg_alt);
}

// After a Newton solve of `it` iterations and `lin_total` Krylov steps: the set the next one runs with
static void update_fieldsplit_policy(Ctx &c, int it, int lin_total, int rc,
                                     std::chrono::steady_clock::time_point t_begin) {
    ++c.fs_solves[c.fs_alt_active ? 1 : 0];
    if ((c.fs_alt_sweeps > 0 || c.amg_alt) && it > 0) {
        // same counts on every rank, so every rank takes the same decision
        const double per_solve = (double)lin_total / it;
        if (!c.fs_measured_policy || (c.comm && c.comm->nranks > 1)) {
            const bool to_alt = !c.fs_alt_active && per_solve >= c.fs_switch_above;
            const bool to_main = c.fs_alt_active && per_solve <= c.fs_back_below;
            if (to_alt || to_main) set_hard_mode(c, to_alt);
        } else if (rc == 0) {
            // measured policy (one GPU): this solve's wall time per Newton iteration goes to the set it ran
            // with; in the hard regime the cheaper set is used, the other one is looked at again now and then
            const int cur = c.fs_alt_active ? 1 : 0;
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count() / it;
            ++c.fs_age[0];
            ++c.fs_age[1];
            if (c.fs_skip_sample) {
                c.fs_skip_sample = false;
            } else {
                c.fs_cost[cur] = c.fs_cost[cur] > 0.0 ? 0.6 * c.fs_cost[cur] + 0.4 * ms : ms;
                c.fs_age[cur] = 0;
            }
            const bool hard_regime = per_solve >= c.fs_switch_above || (c.fs_alt_active && per_solve > c.fs_back_below);
            if (c.fs_probe_left > 0) {
                if (--c.fs_probe_left == 0 && c.fs_cost[1 - cur] > 0.0 && c.fs_cost[1 - cur] <= c.fs_cost[cur])
                    set_hard_mode(c, cur == 0);   // the probed set lost: back to the other one
            } else if (!hard_regime) {
                if (c.fs_alt_active) set_hard_mode(c, false);
            } else if (c.fs_cost[1 - cur] == 0.0 || c.fs_age[1 - cur] >= c.fs_probe_every) {
                c.fs_probe_left = 2;              // (the first solve after the switch does not count)
                set_hard_mode(c, cur == 0);
            } else if (c.fs_cost[1 - cur] < 0.95 * c.fs_cost[cur]) {
                set_hard_mode(c, cur == 0);
            }
        }
    }
}

static int eval_residual(Ctx &c, int mode, double *fnorm) {
    launch_assemble(c, false, mode);
    launch_finalize(c, false, mode);
    launch_norm2(c, c.d_F, 0);
    read_red(c, 1);
    *fnorm = std::sqrt(c.h_red[0]);
    return 0;
}

static void eval_jacobian(Ctx &c, int mode) {
    launch_assemble(c, true, mode);
    launch_finalize(c, true, mode);
}

static void write_report(fedm_newton_report *rep, int it, int lin_total, double fnorm0, double fnorm, int rc) {
    if (!rep) return;
    fedm_newton_report r{};
    r.iterations = it;
    r.linear_iterations = lin_total;
    r.fnorm0 = fnorm0;
    r.fnorm = fnorm;
    r.reason = rc > 0 ? rc : 0;
    r.converged = rc == 0 ? 1 : 0;
    *rep = r;
}

// ---- segregated (uncoupled) step ---------------------------------------------------------------
// Refusals shared by the two stages: nothing is launched.
int segregated_refusal(Ctx &c, const char *who, bool species) {
    if (c.model_kind != 0) {
        set_error(std::string(who) + ": the LMEA family has no segregated step (LFA models with a Poisson row only)");
        return -2;
    }
    if (!c.poisson) {
        set_error("model has no Poisson row");
        return -2;
    }
    if (c.comm || c.n_owned != c.nv) {
        set_error(std::string(who) + ": the segregated step runs on one GPU (this context has a transport or ghost vertices)");
        return -2;
    }
    if (c.photo) {
        set_error(std::string(who) + ": this context has photoionisation set up, whose source tables the segregated step has "
                  "not been tried with (coupled step only: fedm_newton_solve)");
        return -2;
    }
    if (c.diel) {
        set_error(std::string(who) + ": this context has a dielectric layer, whose surface charge is built inside the coupled "
                  "residual (coupled step only: fedm_newton_solve)");
        return -2;
    }
    if (species && c.krylov_scaling != 0) {
        set_error(std::string(who) + ": krylov scaling 'rows' is not defined for the species block (its own equilibration "
                  "is not implemented): set the krylov scaling to 'none'");
        return -2;
    }
    if (species && c.amg && !c.right_precond) {
        set_error(std::string(who) + ": the species solve is flexible GMRES with its preconditioner on the right; this "
                  "context has the field split on the left: set the preconditioner side to 'right'");
        return -2;
    }
    return 0;
}

int ensure_seg_dinv(Ctx &c) {
    if (c.d_seg_dinv) return 0;
    FEDM_HIP_CHECK(hipMalloc((void **)&c.d_seg_dinv, sizeof(double) * (size_t)c.nvp * c.ns * c.ns));
    return 0;
}

}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_residual(fedm_ctx *h, double *F_out, double *fnorm) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    double fn = 0.0;
    eval_residual(c, 0, &fn);
    if (fnorm) *fnorm = fn;
    FEDM_HIP_CHECK(hipGetLastError());   // (a refused launch: before F is copied out)
    if (F_out) return get_vec(c, F_out, c.d_F);
    return 0;
}

int fedm_get_residual(fedm_ctx *h, double *F_out) {
    if (!h || !F_out) return -2;
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    return get_vec(c, F_out, c.d_F);
}

int fedm_jacobian(fedm_ctx *h) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    eval_jacobian(c, 0);
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int64_t fedm_jacobian_nnz(fedm_ctx *h) {
    return h->c.pat.nnz_blocks * h->c.neq * h->c.neq;
}

int fedm_jacobian_csr(fedm_ctx *h, int64_t *indptr, int32_t *indices, double *values) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    const int neq = c.neq, neq2 = neq * neq;
    const size_t nval = (size_t)c.pat.total_bc * SLICE * neq2;
    std::vector<double> val(nval);
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipMemcpy(val.data(), c.d_val, sizeof(double) * nval, hipMemcpyDeviceToHost));
    int64_t pos = 0;
    indptr[0] = 0;
    for (int v = 0; v < c.nv; ++v) {
        const int s = v / SLICE, l = v % SLICE;
        const int len = c.pat.row_len[v];
        for (int cr = 0; cr < neq; ++cr) {
            for (int j = 0; j < len; ++j) {
                const size_t bc = (size_t)c.pat.slice_boff[s] + j;
                const int col = c.pat.colidx[bc * SLICE + l];
                for (int cc = 0; cc < neq; ++cc) {
                    indices[pos] = col * neq + cc;
                    values[pos] = val[(bc * neq2 + cr * neq + cc) * SLICE + l];
                    ++pos;
                }
            }
            indptr[(size_t)v * neq + cr + 1] = pos;
        }
    }
    return 0;
}

int fedm_spmv(fedm_ctx *h, const double *x, double *y) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipMemsetAsync(c.d_tmp, 0, sizeof(double) * c.np, c.stream));
    if (put_vec(c, c.d_tmp, x)) return -1;
    launch_spmv(c, c.d_tmp, c.d_w, false);
    return get_vec(c, y, c.d_w);
}

int fedm_newton_solve(fedm_ctx *h, const fedm_newton_opts *o, fedm_newton_report *rep) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    c.err_cache_comp = -1;
    const auto t_begin = std::chrono::steady_clock::now();
    int it = 0, lin_total = 0, rc = 0;
    double fnorm = 0.0, fnorm0 = 0.0, snorm = 0.0, xnorm = 0.0;
    while (true) {
        // one fused F + J assembly per iteration: the residual norm that decides convergence
        // comes from the same pass (a J assembly is wasted only on the final check)
        // The iteration at which the previous solve converged is expected to be the final check
        // again: assemble the residual only there (a wrong guess costs one extra F+J assembly).
        const bool residual_only = it > 0 && it == c.newton_its_hint;
        if (residual_only) {
            launch_assemble(c, false, 0);
            launch_finalize(c, false, 0);
        } else {
            eval_jacobian(c, 0);
        }
        // |F|, and |dx|, |x| of the previous update (slots 1, 2) in one publication.  After a Jacobian
        // assembly the field split's planes are formed while those numbers travel to the host (an
        // iteration that turns out to be the last one has formed them for nothing: the expected last
        // one assembles no Jacobian at all).
        // at the expected last iteration the watched component's change (adaptive_solver's error norm)
        // rides along: slots 3, 4
        // several GPUs: the update's sums and the error sums are rank-local until this publication's
        // all-reduce carries them with |F|^2 (one collective instead of three)
        const bool sums_local = c.comm && it > 0 && c.red12_local;
        const bool with_error = residual_only && (!c.comm || sums_local) && o->watch_component > 0 &&
                                o->watch_component <= c.neq;
        if (with_error) launch_field_error_slots34(c, o->watch_component - 1);
        norm2_publish(c, c.d_F, 0, with_error ? 5 : 3, sums_local ? (with_error ? 5 : 3) : 1);
        c.red12_local = false;
        bool planes_done = false;
        if (!residual_only && right_preconditioned(c)) {
            prepare_preconditioner_and_rhs(c);
            planes_done = true;
        }
        wait_red(c);
        fnorm = std::sqrt(c.h_red[0]);
        if (it > 0) {
            snorm = std::sqrt(c.h_red[1]);
            xnorm = std::sqrt(c.h_red[2]);
        }
        if (!std::isfinite(fnorm)) {
            rc = FEDM_DIVERGED_NAN;
            break;
        }
        const bool done = it == 0 ? fnorm < o->atol
                                  : (fnorm < o->atol || fnorm <= o->rtol * fnorm0 || snorm < o->stol * xnorm);
        if (it == 0) fnorm0 = fnorm;
        if (done) {
            if (residual_only) ++c.path_stats[PS_RESIDUAL_ONLY_RIGHT];
            if (with_error) {   // the state is final: keep the error norm for fedm_field_error
                c.err_cache = std::sqrt(c.h_red[3]) / std::sqrt(c.h_red[4]);
                c.err_cache_comp = o->watch_component - 1;
            }
            break;
        }
        if (it >= o->max_it) {
            rc = FEDM_DIVERGED_MAX_IT;
            ++c.path_stats[PS_NEWTON_MAX_IT];
            break;
        }
        if (residual_only) ++c.path_stats[PS_RESIDUAL_ONLY_WRONG];
        if (residual_only) eval_jacobian(c, 0);  // not converged after all: the Jacobian is needed
        if (!planes_done) prepare_preconditioner_and_rhs(c);
        int lits = 0;
        double lres = 0.0;
        const bool right = right_preconditioned(c);
        bool updated = false;
        const int lrc = gmres(c, o->ksp_restart, o->ksp_rtol, o->ksp_atol, o->ksp_max_it, &lits, &lres,
                              right ? c.d_F : c.d_rhs, right ? -1.0 : 1.0, right ? fnorm : -1.0, c.d_u, &updated, it);
        lin_total += lits;
        if (lrc != 0 || comm_failed(c)) {
            rc = (lrc < 0 || comm_failed(c)) ? -1 : (lrc == FEDM_DIVERGED_NAN ? FEDM_DIVERGED_NAN : FEDM_DIVERGED_LINEAR);
            break;
        }
        // |dx| and |x| for the stol test (slots 1, 2) are read with the next |F|
        if (!updated) {
            launch_axpy(c, 1.0, c.d_delta, c.d_u);
            launch_norm2(c, c.d_delta, 1);
            launch_norm2(c, c.d_u, 2);
            c.red12_local = false;   // (all-reduced by launch_norm2)
        }
        // ghost entries of the new state: exchanged by the next assembly, behind its interior patches
        if (c.comm && c.assembly_overlap) c.halo_pending = true;
        else comm_halo(c, c.d_u);
        if (comm_failed(c)) {
            rc = -1;
            break;
        }
        ++it;
    }
    if (comm_failed(c)) rc = -1;  // the message is in fedm_last_error (Comm::error)
    if (rc == 0) c.newton_its_hint = it;
    update_fieldsplit_policy(c, it, lin_total, rc, t_begin);
    write_report(rep, it, lin_total, fnorm0, fnorm, rc);
    if (comm_failed(c)) {
        set_error(c.comm->error);
        return -1;
    }
    if (hipGetLastError() != hipSuccess) {
        set_error("HIP error during Newton solve");
        return -1;
    }
    return rc;
}

// Jacobi-preconditioned CG on the potential rows with the species frozen.  The matrix has
// identity rows for species / Dirichlet / padding dofs and their residual is zero once the
// state satisfies the boundary values, so CG runs on the symmetric positive definite
// remainder.  Replaces assemble(a), assemble(L), solve() of fedm-streamer.py:205-215.
int fedm_poisson_solve(fedm_ctx *h, double rtol, int max_it, int *iterations) {
    Ctx &c = h->c;
    c.err_cache_comp = -1;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (!c.poisson) {
        set_error("model has no Poisson row");
        return -2;
    }
    launch_set_dirichlet_state(c);
    launch_assemble(c, true, 1);
    launch_finalize(c, true, 1);
    launch_block_inverse(c);
    launch_scale_copy(c, -1.0, c.d_F, c.d_rhs);   // r = -F
    if (ensure_krylov(c, 1)) return -1;
    const CgResult cg = preconditioned_cg(c, CgMatrix::whole, rtol, max_it);
    launch_axpy(c, 1.0, c.d_V, c.d_u);
    comm_halo(c, c.d_u);
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (iterations) *iterations = cg.it;
    if (comm_failed(c)) {
        set_error(c.comm->error);
        return -1;
    }
    if (!std::isfinite(cg.rn)) return FEDM_DIVERGED_NAN;
    return cg.rn <= rtol * cg.r0 || cg.r0 == 0.0 ? 0 : FEDM_DIVERGED_LINEAR;
}

int fedm_newton_solve_species(fedm_ctx *h, const fedm_newton_opts *o, fedm_newton_report *rep) {
    if (!h || !o) {
        set_error("fedm_newton_solve_species: null argument");
        return -2;
    }
    Ctx &c = h->c;
    if (const int refused = segregated_refusal(c, "fedm_newton_solve_species", true)) return refused;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (ensure_seg_dinv(c)) return -1;
    c.err_cache_comp = -1;
    ++c.seg_stats[SG_SOLVES];
    int it = 0, lin_total = 0, rc = 0;
    double fnorm = 0.0, fnorm0 = 0.0, snorm = 0.0, xnorm = 0.0;
    while (true) {
        // F_u and J_uu in one pass; |F_u| decides (the potential entries of F are zeros).  The iteration at which the
        // previous solve converged is expected to be the final check again: the residual-only twin there (a wrong
        // guess costs the F + J assembly after all), as the coupled loop does.
        const bool residual_only = it > 0 && it == c.seg_newton_its_hint;
        const bool one_pass = launch_assemble_species(c, !residual_only);
        ++c.seg_stats[one_pass ? SG_ONE_PASS : SG_FALLBACK];
        launch_norm2(c, c.d_F, 0);
        read_red(c, 1);
        fnorm = std::sqrt(c.h_red[0]);
        if (!std::isfinite(fnorm)) {
            rc = FEDM_DIVERGED_NAN;
            break;
        }
        const bool done = it == 0 ? fnorm < o->atol
                                  : (fnorm < o->atol || fnorm <= o->rtol * fnorm0 || snorm < o->stol * xnorm);
        if (it == 0) fnorm0 = fnorm;
        if (done) break;
        if (it >= o->max_it) {
            rc = FEDM_DIVERGED_MAX_IT;
            break;
        }
        if (residual_only) {   // not converged after all: the Jacobian is needed
            const bool again = launch_assemble_species(c, true);
            ++c.seg_stats[again ? SG_ONE_PASS : SG_FALLBACK];
        }
        launch_species_block_inverse(c);
        int lits = 0;
        double lres = 0.0;
        const int lrc = species_gmres(c, o->ksp_restart, o->ksp_rtol, o->ksp_atol, o->ksp_max_it, fnorm, &lits, &lres);
        lin_total += lits;
        if (lrc != 0) {
            rc = lrc < 0 ? lrc : (lrc == FEDM_DIVERGED_NAN ? FEDM_DIVERGED_NAN : FEDM_DIVERGED_LINEAR);
            break;
        }
        // u_u += delta_u (delta's potential entries are exact zeros: u_phi keeps its bits); |delta_u|, |u_u| for stol
        launch_axpy(c, 1.0, c.d_delta, c.d_u);
        launch_pick_entries(c, 0, 1.0, c.d_u, c.d_w);
        launch_norm2(c, c.d_delta, 1);
        launch_norm2(c, c.d_w, 2);
        read_red(c, 3);
        snorm = std::sqrt(c.h_red[1]);
        xnorm = std::sqrt(c.h_red[2]);
        ++it;
    }
    c.seg_stats[SG_NEWTON_ITS] += it;
    if (rc == 0) c.seg_newton_its_hint = it;
    write_report(rep, it, lin_total, fnorm0, fnorm, rc);
    if (hipStreamSynchronize(c.stream) != hipSuccess || hipGetLastError() != hipSuccess) {
        set_error("HIP error during the species Newton solve");
        return -1;
    }
    return rc;
}

// The potential stage of the segregated step.  The Poisson rows are linear in the potential, F_phi(u_u, phi) =
// A phi - b(u_u), so one correction A dphi = -F_phi solves them; A = the potential-potential planes as they stand.
// Dirichlet rows: the state takes the boundary values first, their residual is then zero and every CG vector is zero
// there, so the iteration runs on the symmetric positive definite remainder (as fedm_poisson_solve's does).
int fedm_poisson_update(fedm_ctx *h, double rtol, int max_it, int *iterations) {
    if (!h) {
        set_error("fedm_poisson_update: null argument");
        return -2;
    }
    Ctx &c = h->c;
    if (iterations) *iterations = 0;
    if (const int refused = segregated_refusal(c, "fedm_poisson_update", false)) return refused;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    c.err_cache_comp = -1;
    ++c.seg_stats[SG_UPDATES];
    launch_set_dirichlet_state(c);
    if (!c.const_planes_valid && !c.seg_jacobian_done) {
        eval_jacobian(c, 0);   // the context's first Jacobian: writes every plane, the potential-potential one included
        c.seg_jacobian_done = true;
    } else {
        launch_assemble(c, false, 0);
        launch_finalize(c, false, 0);
    }
    launch_pick_entries(c, 1, -1.0, c.d_F, c.d_rhs);   // r = -F_phi, zeros on the species entries
    if (ensure_krylov(c, 1)) return -1;
    const CgResult cg = preconditioned_cg(c, CgMatrix::potential_block, rtol, max_it);
    // the correction has exact zeros on the species entries: they keep their bits
    if (std::isfinite(cg.rn)) launch_axpy(c, 1.0, c.d_V, c.d_u);
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipGetLastError());
    c.seg_stats[SG_CG_ITS] += cg.it;
    if (iterations) *iterations = cg.it;
    if (!std::isfinite(cg.rn)) return FEDM_DIVERGED_NAN;
    return cg.rn <= rtol * cg.r0 ? 0 : FEDM_DIVERGED_LINEAR;
}

int fedm_field_error(fedm_ctx *h, int component, double *rel_err) {
    Ctx &c = h->c;
    if (component < 0 || component >= c.neq) {
        set_error("component out of range");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (component == c.err_cache_comp) {   // computed with the last solve's final residual check
        ++c.path_stats[PS_ERR_CACHE_SERVED];
        *rel_err = c.err_cache;
        return 0;
    }
    launch_field_error(c, component);
    read_red(c, 2);
    *rel_err = std::sqrt(c.h_red[0]) / std::sqrt(c.h_red[1]);
    if (comm_failed(c)) {
        set_error(c.comm->error);
        return -1;
    }
    return 0;
}

int fedm_jacobian_poisson_only(fedm_ctx *h) {
    Ctx &c = h->c;
    if (!c.poisson) {
        set_error("model has no Poisson row");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    launch_set_dirichlet_state(c);
    eval_jacobian(c, 1);
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    return 0;
}

}  // extern "C"
