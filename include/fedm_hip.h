/*
 * fedm_hip.h -- C ABI of libfedm_hip.so: the MI355X (gfx950) replacement for
 * the assemble()/solve() hot path of INP-PM/FEDM.
 *
 * The reference has no FFI; its seam is the DOLFIN subclass protocol
 *     class Problem(df.NonlinearProblem)   F(b, x), J(A, x)   fedm/functions.py:174-202
 * driven by
 *     PETScSNESSolver.solve(problem, x)                       fedm/functions.py:1047
 * Every entry point below names the reference call it replaces.  Plain
 * pointers and sizes only; host pointers are borrowed for the duration of the
 * call; all device memory lives behind the opaque context.
 *
 * Return codes: 0 = ok, <0 = hard error (HIP failure, bad descriptor; see
 * fedm_last_error), >0 = numerical failure (FEDM_DIVERGED_*), which the Python
 * facade turns into RuntimeError so that adaptive_solver's
 * `except Exception` branch (fedm/functions.py:1080-1127) behaves as in the
 * reference.
 *
 * DOF layout: interleaved per vertex, dof = vertex * n_eq + component,
 * species first, potential last (if the model has a Poisson row).
 */
#ifndef FEDM_HIP_H
#define FEDM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEDM_MAX_SPECIES 4
#define FEDM_MAX_TERMS 6
#define FEDM_MAX_REACTIONS 8
#define FEDM_MAX_TAGS 8
#define FEDM_MAX_QP 32
#define FEDM_MAX_FQP 8
#define FEDM_MAX_EXT_NODES 10
#define FEDM_MAX_TABLES 16        /* tabulated coefficient factors of one model (fedm_ctx_create_tabulated)  */
#define FEDM_MAX_TABLE_KNOTS 4096 /* knots of all tables together: 64 KiB of x and y, cache-resident         */

#define FEDM_EQ_REACTION 0                 /* 'reaction'                 functions.py:333 */
#define FEDM_EQ_DIFFUSION_REACTION 1       /* 'diffusion-reaction'                       */
#define FEDM_EQ_DRIFT_DIFFUSION_REACTION 2 /* 'drift-diffusion-reaction'                 */

#define FEDM_BC_ZERO_FLUX 0                /* 'zero flux'                functions.py:472 */
#define FEDM_BC_NEUMANN 1                  /* 'Neumann'                  functions.py:523 */
#define FEDM_BC_FLUX_SOURCE 2              /* 'flux source'              functions.py:514 (fedm_ctx_create_walls) */

#define FEDM_DIVERGED_MAX_IT 1
#define FEDM_DIVERGED_NAN 2
#define FEDM_DIVERGED_LINEAR 3

/* f(E) = sum_i c[i] * E^p[i] * exp(q[i] * E^r[i]); normal form of the deck's
 * 'fun:E' strings (file_input/benchmark_model/transport_coefficients/e_Nb.dat:12).
 * pad_ is the table reference: f(E) = (the sum) * T1(E) [* T2(E)] with piecewise-linear tables handed to
 * fedm_ctx_create_tabulated (the decks' 'Dependence: E/N' files).  Low 16 bits: 1 + index of the first factor,
 * high 16 bits: 1 + index of the second, 0: none -- what every descriptor written before tables existed holds. */
typedef struct {
    int32_t n_terms;
    int32_t pad_;
    double c[FEDM_MAX_TERMS], p[FEDM_MAX_TERMS], q[FEDM_MAX_TERMS], r[FEDM_MAX_TERMS];
} fedm_termsum;

/* What the weak-form builders of fedm/functions.py:219-528 describe symbolically. */
typedef struct {
    int32_t n_species;                       /* balance equations (log variables)          */
    int32_t poisson;                         /* 1: last component is the potential  :379   */
    int32_t axisymmetric;                    /* 1: r = x[0]; 0: r = 0.5/pi          :251   */
    int32_t n_reactions;
    int32_t eq_type[FEDM_MAX_SPECIES];
    double Z[FEDM_MAX_SPECIES];              /* charge number ("sign")              :232   */
    fedm_termsum mu[FEDM_MAX_SPECIES];       /* mobility(|E|)                               */
    fedm_termsum D[FEDM_MAX_SPECIES];        /* diffusion(|E|)                              */
    int32_t has_drift_w[FEDM_MAX_SPECIES];   /* 1: drift velocity is the constant drift_w   */
    double drift_w[FEDM_MAX_SPECIES][2];
    fedm_termsum k[FEDM_MAX_REACTIONS];      /* rate coefficient(|E|)               :839   */
    int32_t power[FEDM_MAX_REACTIONS][FEDM_MAX_SPECIES];   /* power matrix                  */
    int32_t net[FEDM_MAX_REACTIONS][FEDM_MAX_SPECIES];     /* gain - loss           :841    */
    double charge_over_eps;                  /* e/eps0, fedm-streamer.py:248                */
    int32_t n_tags;
    int32_t bc_kind[FEDM_MAX_TAGS][FEDM_MAX_SPECIES];      /* per boundary tag, species     */
    /* quadrature on the reference triangle / unit interval (FIAT "default") */
    int32_t n_qp;
    int32_t n_fqp;
    double qp_x[FEDM_MAX_QP], qp_y[FEDM_MAX_QP], qp_w[FEDM_MAX_QP];
    double fqp_t[FEDM_MAX_FQP], fqp_w[FEDM_MAX_FQP];
    /* Expression sources (P_k nodal values per cell), fedm-tof.py:116 */
    int32_t ext_nodes[FEDM_MAX_SPECIES];     /* 0: none, else nodes per cell (6 for P2)     */
    double ext_B[FEDM_MAX_QP][FEDM_MAX_EXT_NODES];         /* interpolant at qp_x/qp_y      */
    /* 0: unknowns are ln(n) (weak_form_balance_equation_log_representation, every reference example);
     * 1: unknowns are the densities themselves (weak_form_balance_equation(..., log_representation=False),
     *    Flux(..., logarithm_representation=False), fedm/functions.py:219-237, 350-368) */
    int32_t linear_representation;
    int32_t pad2_;
} fedm_model_desc;

/* The walls of an LFA model: what Boundary_flux('flux source', ...) adds to fedm_model_desc for the entries of
 * bc_kind that hold FEDM_BC_FLUX_SOURCE (fedm/functions.py:514-522, fedm-gd.py:346-351); handed to
 * fedm_ctx_create_walls next to the model, which does not change. */
typedef struct {
    double vth[FEDM_MAX_TAGS][FEDM_MAX_SPECIES];   /* thermal velocity [m/s], >= 0                          */
    double ref[FEDM_MAX_TAGS][FEDM_MAX_SPECIES];   /* reflection coefficient, 1 + ref != 0                  */
    double gamma[FEDM_MAX_TAGS];                   /* secondary emission coefficient of the tag             */
    int32_t emits[FEDM_MAX_SPECIES];               /* 1: receives the secondaries (particle_type 'electrons') */
    int32_t is_ion[FEDM_MAX_SPECIES];              /* 1: summed into Ion_flux = sum max(Gamma_i . n, 0)     */
} fedm_wall_desc;

typedef struct {
    int32_t n_vertices;
    int32_t n_cells;
    const double *coords;        /* [n_vertices][2] = (r, z)                               */
    const int32_t *cells;        /* [n_cells][3]                                           */
    const int8_t *facet_tags;    /* [n_cells][3], facet i opposite vertex i; 0 = none      */
    int32_t n_dirichlet;         /* DirichletBC rows, fedm-streamer.py:233.  A dof of a ghost
                                    vertex with identity rows (below) may be listed: its row
                                    stays an identity row with F = 0                        */
    const int32_t *dirichlet_dofs;
    const double *dirichlet_vals;
    int32_t n_owned_vertices;    /* multi-GPU: vertices [0, n_owned) are owned, the rest are
                                    ghosts of neighbouring partitions; 0 = all owned        */
    /* Deep halos (several ghost layers, fedm_amd/partition.py): the ghost vertices whose rows are
     * identity rows -- the outermost layer.  The rows of all other ghost vertices are assembled
     * like owned rows (redundantly), so that a vector exchanged once stays exact on the owned rows
     * through as many operator applications as there are layers.  NULL: every ghost row is an
     * identity row (one ghost layer).  halo_depth: the number of layers (1 with NULL). */
    int32_t n_identity_vertices;
    const int32_t *identity_vertices;
    int32_t halo_depth;
} fedm_mesh_desc;

typedef struct {
    double rtol, atol, stol;     /* SNES: fedm-streamer.py:295; DOLFIN defaults 1e-10, 1e-16 */
    int32_t max_it;              /* :297                                                    */
    int32_t ksp_restart;         /* GMRES restart (PETSc default 30)                        */
    double ksp_rtol;             /* PETSc default 1e-5, on the preconditioned residual      */
    double ksp_atol;
    int32_t ksp_max_it;          /* PETSc default 10000                                     */
    int32_t watch_component;     /* 1 + the component whose relative change fedm_field_error will be
                                    asked for right after this solve (adaptive_solver's error norm,
                                    fedm/functions.py:1062-1064); 0: none.  Its two sums then ride on the
                                    publication of the final residual check: no extra round trip to the
                                    host.  (One GPU; was padding: 0 keeps the old behaviour.)          */
} fedm_newton_opts;

typedef struct {
    int32_t iterations;          /* Newton iterations taken                                */
    int32_t converged;
    int32_t linear_iterations;   /* total GMRES iterations                                 */
    int32_t reason;              /* 0 or FEDM_DIVERGED_*                                   */
    double fnorm0, fnorm;        /* |F| before / after                                     */
} fedm_newton_report;

/* scalar CSR matrix handed across the boundary (multigrid operators, mass matrix) */
typedef struct {
    int32_t n_rows, n_cols;
    const int64_t *indptr;
    const int32_t *indices;
    const double *values;
} fedm_csr;

/* ---- LMEA model family (glow discharge, examples/glow_discharge/fedm-gd.py) --------------
 * Components: 0 = ln(electron energy density), 1..n_species-1 = ln(number density) of the
 * species with an equation (species 0, the background gas, has none), last = potential.
 * Transport and rate coefficients are nodal P1 fields refreshed by the caller every step
 * (Transport_/Rate_coefficient_interpolation, fedm/functions.py:531-750) and linearised in the
 * mean electron energy on the device (semi_implicit_coefficients, :753-774). */
#define FEDM_GD_MAX_SPECIES 6
#define FEDM_GD_MAX_REACTIONS 16
typedef struct {
    int32_t n_species;                        /* including the background gas            */
    int32_t n_reactions;
    int32_t n_tags;
    int32_t axisymmetric;
    double N0;                                /* gas number density, exp_u[0] in Source_term */
    double charge_over_eps;
    int32_t eq_type[FEDM_GD_MAX_SPECIES];     /* per species (index 0 unused)            */
    int32_t grad_diffusion[FEDM_GD_MAX_SPECIES];
    int32_t is_ion[FEDM_GD_MAX_SPECIES];      /* contributes to Ion_flux, fedm-gd.py:351 */
    double sign[FEDM_GD_MAX_SPECIES];
    double vth[FEDM_GD_MAX_SPECIES];          /* heavy species thermal velocity          */
    double vth_e_coef;                        /* 16 e / (3 pi m_e): vth_e = sqrt(coef * mean energy) */
    int32_t power[FEDM_GD_MAX_REACTIONS][FEDM_GD_MAX_SPECIES];
    int32_t net[FEDM_GD_MAX_REACTIONS][FEDM_GD_MAX_SPECIES];
    double energy_loss[FEDM_GD_MAX_REACTIONS];   /* the decks' two sentinel values stay what they are: 7.77e77 ->
                                                  * (energy_Ei - mean energy), 9.99e99 -> mean energy, :906-909      */
    double ref[FEDM_MAX_TAGS][FEDM_GD_MAX_SPECIES];   /* reflection coefficients         */
    double gamma[FEDM_MAX_TAGS];              /* secondary emission coefficient          */
    double we_secondary;                      /* mean energy of secondary electrons [eV] */
    int32_t n_qp, n_fqp;
    double qp_x[FEDM_MAX_QP], qp_y[FEDM_MAX_QP], qp_w[FEDM_MAX_QP];
    double fqp_t[FEDM_MAX_FQP], fqp_w[FEDM_MAX_FQP];
    /* Energy_Source_term's `Ei` and `mean_energy` arguments (fedm/functions.py:855, 906-909), used by reactions whose
     * energy_loss is a sentinel only.  mean_energy_form: FEDM_GD_ME_UNKNOWN_RATIO = the expression the reference's
     * scripts pass, u[0] / u[n - 1] -- the ratio of the energy and the electron UNKNOWNS at the point, as written
     * (examples/glow_discharge/fedm-gd.py:358) -- differentiated like every other term of the form.  A numeric
     * mean_energy never reaches the device: the host folds it into energy_loss. */
    double energy_Ei;
    int32_t mean_energy_form;
} fedm_gd_desc;
#define FEDM_GD_ME_NONE 0
#define FEDM_GD_ME_UNKNOWN_RATIO 1

/* nodal fields of fedm_gd_set_fields, in this order, each [n_vertices]:
 *   mu[n_species], D[n_species], mu_diff[n_species], D_diff[n_species],
 *   k[n_reactions], k_diff[n_reactions], mean_energy_old, mean_energy, u_e_old           */
#define FEDM_GD_N_FIELDS(ns, nr) (4 * (ns) + 2 * (nr) + 3)

/* Per-step refresh of the LMEA coefficient fields on the device (what the script does on the
 * host between solves, examples/glow_discharge/fedm-gd.py:424-443,452): one "program" per
 * field row of fedm_gd_set_fields. */
#define FEDM_GDP_KEEP 0      /* leave the row as uploaded ('const' dependence, set once)            */
#define FEDM_GDP_TABLE 1     /* np.interp(arg, table) * scale      functions.py:627-630, 739-747    */
#define FEDM_GDP_SCALED_ROW 2 /* scale * fields[src_row]           'ESR': kB*Tgas*mu/e, :633        */
#define FEDM_GDP_ME_OLD 3    /* mean_energy_old <- mean_energy     fedm-gd.py:426-427               */
#define FEDM_GDP_ME 4        /* mean_energy (updated after the solve, fedm-gd.py:452)               */
#define FEDM_GDP_UE_OLD 5    /* ln n_e of the previous step (u_oldV[-1], fedm-gd.py:424)             */
#define FEDM_GDP_ARG_ENERGY 0   /* mean_energy_old */
#define FEDM_GDP_ARG_REDFIELD 1 /* reduced electric field project(1e21*|grad Phi|/N0), :432          */
typedef struct {
    int32_t kind, table, arg, src_row;
    double scale;
} fedm_gd_field_prog;

typedef struct fedm_ctx fedm_ctx;

const char *fedm_last_error(void);
/* Version of this header's structs and entry points; a binding compares it with the constant it was
 * written against and refuses a library of another version (a descriptor that grew would otherwise be
 * read past its end).  2: fedm_model_desc.linear_representation, fedm_newton_opts.watch_component,
 * fedm_pattern_stats out[12], fedm_debug_comm_fault out[6], fedm_pattern_info, fedm_mesh_desc's deep-halo fields.
 * 3: fedm_fieldsplit_tiles_info, fedm_fieldsplit_tiles_stats, fedm_debug_fieldsplit_apply, fedm_debug_fieldsplit_tiles.
 * 4: fedm_state_snapshot, fedm_state_restore; fedm_fieldsplit_tiles_stats out[10]; fedm_comm_stats out[10]; fedm_fieldsplit_policy.
 * 5: fedm_gd_desc.energy_Ei, .mean_energy_form (the sentinel energy losses on the device); fedm_debug_species_planes_check;
 *    fedm_time_kernel kinds 4, 5; fedm_pattern_info out[9].
 * 6: fedm_debug_fieldsplit_apply_operator, fedm_debug_fieldsplit_apply_produced.
 * 7: fedm_launched_assembly, fedm_get_residual; fedm_pattern_info out[6..7] predict what the next fedm_jacobian
 *    launches.
 * 8: fedm_solver_path_stats, fedm_debug_linear_solve.
 * 9: fedm_set_krylov_scaling, fedm_get_krylov_scaling; additive: fedm_poisson_update, fedm_newton_solve_species,
 *    fedm_segregated_stats, fedm_debug_species_linear_solve, fedm_debug_species_assembly, fedm_debug_block_product, fedm_time_kernel kinds 6, 7.
 * 10: fedm_debug_gd_reduced_field, fedm_debug_get_ext_source; fedm_gd_prep_setup refuses what np.interp refuses (a
 *    looked-up table without entries, a tab_ptr that does not start at 0 or decreases, null table arrays, a program
 *    kind or argument outside its enum).  Additive under 10 (no struct changes size or offsets, no signature changes):
 *    fedm_ctx_create_tabulated; fedm_termsum.pad_, which had to be 0, is the table reference.  fedm_ctx_create_walls
 *    with fedm_wall_desc; FEDM_BC_FLUX_SOURCE, a value of bc_kind that the two older creators refuse.
 *    fedm_photo_setup with fedm_photo_desc and fedm_photo_hierarchy, fedm_photo_update, fedm_photo_get, fedm_photo_stats.
 *    fedm_diag_setup and fedm_diagnostics with fedm_diag_opts and fedm_diag.
 *    fedm_fields_setup, fedm_probe_setup and fedm_fields with fedm_field_req and fedm_field_opts.
 *    fedm_gd_balance_setup and fedm_gd_balance with fedm_gd_balance.
 *    fedm_gd_fields_setup, fedm_gd_probe_setup and fedm_gd_fields with the FEDM_GD_FIELD_* kinds.
 *    fedm_currents_setup, fedm_currents_solve, fedm_currents_get_psi and fedm_currents with fedm_currents.
 *    fedm_circuit_setup, fedm_circuit_measure, fedm_circuit_advance and fedm_circuit_get with fedm_circuit_desc and
 *    fedm_circuit_state.
 *    fedm_ctx_create_dielectric, fedm_dielectric_set_voltage, fedm_dielectric_accept, fedm_dielectric_get and
 *    fedm_dielectric_set with fedm_dielectric_desc and fedm_dielectric_totals. */
#define FEDM_ABI_VERSION 10
int fedm_abi_version(void);

/* mesh + model -> device: colouring, sliced block-ELL pattern, buffers.
 * Replaces FunctionSpace/derivative/Problem set-up, fedm-streamer.py:133-291. */
int fedm_ctx_create(const fedm_mesh_desc *mesh, const fedm_model_desc *model, int device,
                    fedm_ctx **out);
/* fedm_ctx_create for a model whose coefficients carry table references (fedm_termsum.pad_): n_tables
 * piecewise-linear tables laid out as fedm_gd_prep_setup's -- concatenated knots tab_x [V/m] and values tab_y with
 * tab_ptr[n_tables + 1], starting at 0 and not decreasing.  The element routines look a factor up at the cell's own
 * |E| (P1: constant per cell): np.interp's value -- tab_y's first / last entry outside the knots -- and the exact
 * derivative, the segment's slope inside [first knot, last knot) and 0 outside, so the Jacobian stays the exact
 * Gateaux derivative.  (The reference looks E/N tables up per NODE at the projected field of the previous step,
 * fedm/functions.py:629-630; that lagged form is what the LMEA family does here, fedm_gd_prep_setup.)
 * Refused (-2, nothing allocated, fedm_last_error names the table): more than FEDM_MAX_TABLES tables or
 * FEDM_MAX_TABLE_KNOTS knots in all, a reference beyond n_tables, a table without entries, knots that do not strictly
 * increase, a knot or value that is not finite, a tab_ptr that does not start at 0 or decreases, null arrays with
 * entries, a reference in a model without the Poisson equation (there is no |E|).  fedm_ctx_create is this call with
 * no tables: it refuses any reference.  Models with a reference run the second-generation assembly (variants 1, 2 of
 * fedm_pattern_info; 0 by global colouring), never the one-pass kernels. */
int fedm_ctx_create_tabulated(const fedm_mesh_desc *mesh, const fedm_model_desc *model, int n_tables,
                              const int32_t *tab_ptr, const double *tab_x, const double *tab_y, int device,
                              fedm_ctx **out);
/* fedm_ctx_create_tabulated for a model with 'flux source' walls: walls describes every (tag, species) whose bc_kind
 * is FEDM_BC_FLUX_SOURCE (null: no walls; n_tables = 0: no tables).  On a facet of such a tag, species s adds
 *   2 pi r v [ (1 - ref)/(1 + ref) (vth/2 + |Z mu(|E|) E.n|) n_s  -  2 gamma/(1 + ref) sum_(i: is_ion) max(Gamma_i.n, 0) ] ds
 * to its row: the drift part for 'drift-diffusion-reaction' only, the emission part for a drift-diffusion species
 * with emits, nothing for 'reaction'; Gamma_i.n = -D_i grad(n_i).n + Z_i mu_i E.n n_i.  The Jacobian is the exact
 * derivative with d|x| = sign(x), sign(0) = 1, and max(x, 0) = (x + |x|)/2, as the LMEA kernels take them.
 * With gamma != 0 the Jacobian planes (emitting species, ion) count as coupled (fedm_plane_masks).
 * Refused (-2, nothing allocated, fedm_last_error names tag and species): ref not finite or 1 + ref == 0; vth
 * negative or not finite; gamma not finite; a 'flux source' entry in a model without the Poisson equation (the facet
 * kernels exist for models with one; there is no E); a 'flux source' drift-diffusion species with has_drift_w;
 * gamma != 0 on a tag none of whose 'flux source' species has emits; a 'flux source' entry without walls, which is
 * what fedm_ctx_create and fedm_ctx_create_tabulated -- this call without walls -- meet.  Wall models run the
 * second-generation assembly (variants 1, 2 of fedm_pattern_info; 0 by global colouring), never the one-pass
 * kernels. */
int fedm_ctx_create_walls(const fedm_mesh_desc *mesh, const fedm_model_desc *model, const fedm_wall_desc *walls,
                          int n_tables, const int32_t *tab_ptr, const double *tab_x, const double *tab_y, int device,
                          fedm_ctx **out);
int fedm_ctx_create_gd(const fedm_mesh_desc *mesh, const fedm_gd_desc *model, int device,
                       fedm_ctx **out);
int fedm_gd_set_fields(fedm_ctx *ctx, const double *fields /* [n_fields][n_vertices] */);
/* mass: consistent P1 mass matrix (Cartesian dx) for project(); tables: concatenated x/y with
 * tab_ptr[n_tables+1]; progs: one per field row */
int fedm_gd_prep_setup(fedm_ctx *ctx, const fedm_csr *mass, int n_tables, const int32_t *tab_ptr,
                       const double *tab_x, const double *tab_y, const fedm_gd_field_prog *progs);
int fedm_gd_prep_step(fedm_ctx *ctx);            /* after fedm_shift_state, before the solve   */
int fedm_gd_update_mean_energy(fedm_ctx *ctx);   /* mean_energy = exp(u_0 - u_e), :452         */
int fedm_gd_get_fields(fedm_ctx *ctx, double *out /* [n_fields][n_vertices] */);
/* Test hook: the projected reduced electric field of the last fedm_gd_prep_step (the argument of the E/N look-ups),
 * n_vertices entries in the device's vertex order.  -2 when the context is not LMEA or has no refresh pipeline. */
int fedm_debug_gd_reduced_field(fedm_ctx *ctx, double *out /* [n_vertices] */);
void fedm_ctx_destroy(fedm_ctx *ctx);

/* u_new / u_old / u_old1 (N doubles each, any may be NULL to leave unchanged).
 * Replaces Function.assign / rev_assigner.assign, fedm-streamer.py:282-283,306-307. */
int fedm_set_state(fedm_ctx *ctx, const double *u_new, const double *u_old, const double *u_old1);
int fedm_get_state(fedm_ctx *ctx, double *u_new);
int fedm_get_state_old(fedm_ctx *ctx, double *u_old);
/* u_old1 <- u_old; u_old <- u_new on the device (fedm-streamer.py:306-307) */
int fedm_shift_state(fedm_ctx *ctx);
/* u_new <- u_old (step rejection, fedm/functions.py:1103) */
int fedm_reset_state(fedm_ctx *ctx);
/* The three resident states kept in / brought back from a device-side copy (no host transfer): a
 * checkpoint of the time loop, what a script does with Function.copy(deepcopy=True) before a
 * speculative step.  bench.py repeats its timed window from one. */
int fedm_state_snapshot(fedm_ctx *ctx);
int fedm_state_restore(fedm_ctx *ctx);

/* dt.time_step / dt_old.time_step, fedm/functions.py:350 */
int fedm_set_step(fedm_ctx *ctx, double dt, double dt_old);
/* time-dependent Dirichlet values (time_dependent_arguments, functions.py:1042-1044) */
int fedm_set_dirichlet_values(fedm_ctx *ctx, const double *vals);
/* Expression source of one species for this step: [n_cells][ext_nodes] */
int fedm_set_ext_source(fedm_ctx *ctx, int species, const double *nodal);
/* The same source evaluated on the device.  A DOLFIN Expression string of the arithmetic subset
 * (examples/time_of_flight/fedm-tof.py:116: f = Expression('exp(-(pow(x[1]-w*t, 2)+...)...', D=..., w=...,
 * t=t, degree=2); the script advances f.t before every solve, :145) is handed over once as a postfix
 * program over x[0], x[1], constants and named parameters; fedm_ext_source_eval then fills the
 * species' [n_cells][ext_nodes] table at the P_degree lattice nodes of every cell with the current
 * parameter values -- what fedm_set_ext_source does with a host array, without the host evaluation and
 * the upload.  ops: n_ops pairs (opcode, argument). */
#define FEDM_EXPR_MAX_OPS 256
#define FEDM_EXPR_MAX_PARAMS 16
#define FEDM_EXPR_STACK 24
enum {
    FEDM_OP_CONST = 0, /* push consts[arg]   */
    FEDM_OP_X = 1,     /* push x[arg]        */
    FEDM_OP_PARAM = 2, /* push params[arg]   */
    FEDM_OP_ADD = 3, FEDM_OP_SUB = 4, FEDM_OP_MUL = 5, FEDM_OP_DIV = 6, FEDM_OP_POW = 7, /* binary */
    FEDM_OP_NEG = 8, FEDM_OP_EXP = 9, FEDM_OP_LOG = 10, FEDM_OP_SQRT = 11, FEDM_OP_SIN = 12, FEDM_OP_COS = 13,
    FEDM_OP_TAN = 14, FEDM_OP_FABS = 15, FEDM_OP_TANH = 16, FEDM_OP_ATAN = 17 /* unary */
};
int fedm_ext_source_program(fedm_ctx *ctx, int species, int n_ops, const int32_t *ops /* [n_ops][2] */,
                            int n_consts, const double *consts, int n_params);
int fedm_ext_source_eval(fedm_ctx *ctx, int species, const double *params /* [n_params] */);
/* Test hook: the species' [n_cells][ext_nodes] table as it stands on the device (after fedm_set_ext_source or
 * fedm_ext_source_eval); refused (-2) where fedm_set_ext_source is. */
int fedm_debug_get_ext_source(fedm_ctx *ctx, int species, double *out /* [n_cells][ext_nodes] */);

/* Problem.F: assemble(F) then bc.apply(b, x)              fedm/functions.py:188-194 */
int fedm_residual(fedm_ctx *ctx, double *F_out /* N or NULL */, double *fnorm /* or NULL */);
/* Problem.J: assemble(J) then bc.apply(A)                 fedm/functions.py:196-202
 * (also assembles F).  csr_* NULL -> stay on device. */
int fedm_jacobian(fedm_ctx *ctx);
/* pattern/values of the assembled Jacobian as scalar CSR, for parity tests */
int64_t fedm_jacobian_nnz(fedm_ctx *ctx);
int fedm_jacobian_csr(fedm_ctx *ctx, int64_t *indptr, int32_t *indices, double *values);
/* y = J x with the assembled Jacobian (KSP mat-vec), for parity tests and bench */
int fedm_spmv(fedm_ctx *ctx, const double *x, double *y);

/* nonlinear_solver.solve(problem, u_new.vector())         fedm/functions.py:1047 */
int fedm_newton_solve(fedm_ctx *ctx, const fedm_newton_opts *opts, fedm_newton_report *rep);
/* Poisson row only, species frozen (initial potential, fedm-streamer.py:205-215) */
int fedm_poisson_solve(fedm_ctx *ctx, double rtol, int max_it, int *iterations);

/* ---- segregated (uncoupled) time step ------------------------------------------------------
 * The reference's second solution strategy: the potential on its own with the densities frozen, then the species
 * among themselves with the field frozen.  One step from the shifted state is fedm_poisson_update followed by
 * fedm_newton_solve_species.  First order in dt against the coupled step; explicit in the space charge, so stable
 * for dt below the dielectric relaxation time eps0 / (e mu_e n_e).  One GPU, LFA family with a Poisson row. */

/* Poisson_solver(A, L, b, u, bcs) (fedm/functions.py:1154-1161) once per step: the potential entries of u_new are
 * solved from the Poisson rows with the species entries of u_new frozen (bit-identical afterwards); Dirichlet rows
 * stay as they are.  The right-hand side comes from a residual-only assembly; the operator is the potential-potential
 * planes of the Jacobian as they stand (assembled once if this context has never assembled a Jacobian) and the
 * preconditioner the installed multigrid hierarchy (Jacobi without one): conjugate gradients to
 * |r| <= rtol |r0|.  iterations (unless NULL): CG steps.  Returns 0, FEDM_DIVERGED_LINEAR or FEDM_DIVERGED_NAN. */
int fedm_poisson_update(fedm_ctx *ctx, double rtol, int max_it, int *iterations);
/* nonlinear_solver.solve on the species equations alone, what a script gets from Source_term / Energy_Source_term
 * with coupling='uncoupled' (fedm/functions.py:777-843, 845-912) and a problem without the Poisson equation: Newton
 * (newtonls / basic, the rules of fedm_newton_solve) on the species rows with the potential entries frozen
 * (bit-identical afterwards).  Each system J_uu delta_u = -F_u goes to flexible GMRES(ksp_restart) preconditioned by
 * the species polynomial of fedm_set_fieldsplit (point-block Jacobi on the n_species x n_species blocks when none is
 * installed), no V-cycle; ksp_rtol / ksp_atol are tested on the true species residual, which is formed before a
 * solve reports success.  The report's norms are norms over the species entries.  Assembly: the species-only
 * one-pass kernels where they apply (csrc/assemble3.hip: neither the Poisson row nor a plane of the potential row or
 * column is evaluated, accumulated or written; F of the potential rows is written as 0); otherwise the full assembly,
 * whose potential row and column the solve ignores. */
int fedm_newton_solve_species(fedm_ctx *ctx, const fedm_newton_opts *opts, fedm_newton_report *rep);
/* Counters of the two calls above since the context was created (or the last call with reset != 0; out may be NULL
 * then): out = {potential updates, their CG iterations, species solves, species-only one-pass assemblies, fallback
 * (full) assemblies run for species solves, species Newton iterations, species Krylov steps, reserved}. */
int fedm_segregated_stats(fedm_ctx *ctx, int64_t out[8], int reset);
/* Test hooks.  fedm_debug_species_assembly: the assembly a species Newton iteration runs, alone -- F_u and J_uu
 * (jacobian != 0) or F_u by the residual-only twin (jacobian = 0: the matrix is not touched); F of the potential rows is
 * 0 either way.  Returns 1 when the species-only one-pass kernel ran, 0 when the full assembly did (counted in
 * fedm_segregated_stats like a solve's assemblies), < 0 on refusal.
 * fedm_debug_block_product: y = J_bb x_b with the Jacobian as it stands, block 0 = species (y_u = J_uu x_u, the
 * structurally zero species planes skipped), 1 = potential (y_phi = J_phiphi x_phi); the entries of the other block come
 * back as exact zeros.  Host vectors in the caller-side layout of fedm_residual: the products the two stages make. */
int fedm_debug_species_assembly(fedm_ctx *ctx, int jacobian);
int fedm_debug_block_product(fedm_ctx *ctx, int which, const double *x, double *y);
/* Test hook, fedm_debug_linear_solve's counterpart for the species block: x = the flexible-GMRES solution of
 * J_uu x_u = b_u with the Jacobian as the last species assembly (or fedm_jacobian) left it, through the very call
 * fedm_newton_solve_species makes (opts' ksp_* fields are read).  b and x in the caller-side layout of fedm_residual;
 * the potential entries of b are ignored, those of x come back as zeros.  The state is not touched; F of the last
 * assembly is overwritten with -b_u.  Returns what the solver returns; its / rnorm: its step count and the true
 * residual norm |b_u - J_uu x_u|_2 it reports. */
int fedm_debug_species_linear_solve(fedm_ctx *ctx, const double *b, const fedm_newton_opts *opts, double *x, int *its,
                                    double *rnorm);

/* ---- photoionisation: Helmholtz sources on the device -----------------------------------------
 * The three-term Helmholtz approximation of the photoionisation integral (Bourdon et al. 2007; case 3 of Bagheri et
 * al. 2018): with R = sum_(j in src_reaction) k_j(|E|) prod_i n_i^power[j][i], the rate of the designated reactions,
 *     S_ph = sum_m c[m] y_m,      (-lap + kappa[m]^2) y_m = efficiency R,
 * weak form  int (grad y . grad v + kappa^2 y v) w dx = int efficiency R v w dx  with w = x[0] for an axisymmetric model
 * and 1 otherwise, y = 0 on the vertices of the facets whose tag is in zero_tag_mask (bit tag - 1), zero flux elsewhere.
 * S_ph goes into the degree-1 source tables (ext_nodes = 3) of the species in target_species_mask, which the element
 * routines add to those species' rows as they add an Expression source.
 * Explicit lag: R is evaluated at u_old -- densities exp(u_old) (u_old itself in the linear representation), |E| of
 * u_old's potential, rate coefficients once per cell as the element routines evaluate them, the model's quadrature
 * rule -- so the source is frozen during a Newton solve and the Jacobian stays exact.  First order in dt.  The mass
 * matrix is the consistent one: S_ph may undershoot zero slightly where kappa h is large; it enters the balance
 * linearly and is neither lumped nor clipped.
 * One GPU, LFA family, coupled step (fedm_newton_solve): fedm_poisson_update and fedm_newton_solve_species refuse a
 * context with photoionisation set up. */
typedef struct {
    int32_t n_terms;                             /* 1..4                                                    */
    int32_t n_src;                               /* 1..FEDM_MAX_REACTIONS designated ionisation reactions   */
    double c[4];                                 /* [1/m^2]                                                 */
    double kappa[4];                             /* [1/m], > 0                                              */
    double efficiency;
    int32_t src_reaction[FEDM_MAX_REACTIONS];    /* indices into fedm_model_desc.k                          */
    uint32_t target_species_mask;                /* bit s: species s receives S_ph                          */
    uint32_t zero_tag_mask;                      /* bit t - 1: y = 0 on the vertices of the facets tagged t */
} fedm_photo_desc;
/* One term's preconditioner, as fedm_amg_setup takes the potential block's: A[0] is the term's operator
 * K_w + kappa^2 M_w in the context's vertex numbering with the rows and columns of the zero vertices eliminated
 * symmetrically (unit diagonal), kept in double precision as the operator of the conjugate gradients; the levels
 * below precondition them with plain V(nu,nu) cycles of damped Jacobi (nu > 0).  n_levels = 1: Jacobi alone (P, R and
 * coarse_inverse are not read). */
typedef struct {
    int32_t n_levels, nu;
    const fedm_csr *A, *P, *R;
    const double *coarse_inverse;
    double omega;
} fedm_photo_hierarchy;
/* Refused (-2, nothing installed, fedm_last_error says why): an LMEA context; a context with ghost vertices or a
 * transport; n_terms outside 1..4; kappa <= 0 or not finite; n_src outside 1..FEDM_MAX_REACTIONS or a reaction index
 * outside the model's; no target species, a target beyond the model's species, one without a degree-1 source table or
 * one with an Expression program; a tag bit beyond the model's tags; a hierarchy that fedm_amg_setup would refuse.
 * Replaces an earlier set-up; every y_m starts at 0. */
int fedm_photo_setup(fedm_ctx *ctx, const fedm_photo_desc *desc, const fedm_photo_hierarchy *terms /* [n_terms] */);
/* Load vector g_a = int efficiency R phi_a w from u_old (once for all terms; summed per vertex in a fixed order, no
 * atomics: bitwise reproducible), then per term conjugate gradients warm-started from the previous update's y_m until
 * |r|_2 <= rtol |g|_2 on the recurrence's residual (0 iterations when the start already satisfies it), then the
 * targets' tables ext[cell][a] = sum_m c[m] y_m[vertex a of cell].  iterations (unless NULL): CG steps per term.
 * Returns 0, FEDM_DIVERGED_LINEAR (a term stopped at max_it; the tables are written all the same) or FEDM_DIVERGED_NAN
 * (a state that is not finite, or an operator that is not positive definite: the terms it met are set back to 0, so the
 * tables written are finite and the next update starts clean; no new set-up is needed). */
int fedm_photo_update(fedm_ctx *ctx, double rtol, int max_it, int iterations[4]);
/* Test hook: the solutions y[n_terms][n_vertices] and the load vector g[n_vertices] of the last update (either may be
 * NULL), in the context's vertex numbering. */
int fedm_photo_get(fedm_ctx *ctx, double *y, double *g);
/* out = {updates, CG iterations of term 0, 1, 2, 3, V-cycles, terms that stopped at max_it, reserved} since the set-up
 * (or the last call with reset != 0; out may be NULL then). */
int fedm_photo_stats(fedm_ctx *ctx, int64_t out[8], int reset);

/* ---- linear solver set-up -----------------------------------------------------------------
 * The reference hands J dx = -F to MUMPS (examples) or to PETSc GMRES + default PC (test
 * harness, tests/integrated_tests/streamer_discharge/fedm_streamer.py:32).  Here: GMRES with
 * point-block Jacobi on the species rows and, when a hierarchy has been installed, one
 * multigrid V-cycle on the (constant) potential block, combined block-triangularly. */

/* scalar CSR of block component (cr, cc) of the assembled Jacobian (n_vertices rows) */
int64_t fedm_block_nnz(fedm_ctx *ctx);
int fedm_block_csr(fedm_ctx *ctx, int cr, int cc, int64_t *indptr, int32_t *indices,
                   double *values);
/* assemble only the Poisson row with the species frozen (identity species rows) */
int fedm_jacobian_poisson_only(fedm_ctx *ctx);
/* install a multigrid hierarchy for the potential block: n_levels operators A[l]
 * (A[0] = fine), n_levels-1 prolongators P[l] (rows of level l, cols of level l+1) and
 * their transposes R[l]; dense inverse of the coarsest operator (NULL when
 * fedm_amg_set_global_hierarchy takes over below the finest level); V(nu,nu) cycles with damped
 * Jacobi smoothing, nu < 0 selects V(0,|nu|) (no pre-smoothing). */
int fedm_amg_setup(fedm_ctx *ctx, int n_levels, const fedm_csr *A, const fedm_csr *P,
                   const fedm_csr *R, const double *coarse_inverse, int nu, double omega);
int fedm_amg_clear(fedm_ctx *ctx);
/* several GPUs: the hierarchy installed with fedm_amg_setup holds the rank's finest level and its
 * level-1 space only (coarse_inverse = NULL there).  The ranks' level-1 spaces are concatenated
 * (n_global unknowns, this rank's start at `offset`) and everything below is ONE global
 * hierarchy, replicated on every rank: A[0] is the Galerkin operator of the undecomposed
 * potential block on that space.  A V-cycle exchanges the finest level's ghost values twice and
 * all-reduces the level-1 right-hand side once. */
int fedm_amg_set_global_hierarchy(fedm_ctx *ctx, int n_global, int offset, int n_levels,
                                  const fedm_csr *A, const fedm_csr *P, const fedm_csr *R,
                                  const double *coarse_inverse, int nu, double omega);
/* The same hierarchy with a polynomial smoother: `degree` Richardson sweeps x += w Dinv (b - A x)
 * per leg, weights[level * degree + i] in the order of the pre-smoother (the post-smoother runs them
 * backwards: the cycle stays symmetric for the Poisson-only CG); Chebyshev roots on
 * [lambda_max / a, lambda_max] of Dinv A are the intended choice.  Costs two more streams of the
 * finest operator per cycle at degree 2 (the coarse levels stay two kernels each: the polynomial is
 * folded into their composite matrices) and contracts 0.38 instead of 0.68 per cycle on the bench
 * mesh.  as_alternative = 0: replaces the hierarchy of fedm_amg_setup.  1: installed next to it and
 * used together with the alternative species sweeps (fedm_set_fieldsplit_alternative: Newton solves
 * that need many Krylov steps), one GPU only. */
int fedm_amg_setup_poly(fedm_ctx *ctx, int n_levels, const fedm_csr *A, const fedm_csr *P,
                        const fedm_csr *R, const double *coarse_inverse, int degree,
                        const double *weights, int as_alternative);
/* Richardson sweeps z += w_k Duu^-1 (r - Juu z) on the species block inside the field split;
 * one weight per sweep (equal weights = damped block Jacobi, Chebyshev roots = polynomial) */
int fedm_set_fieldsplit(fedm_ctx *ctx, int sweeps, const double *weights);
/* A second set of sweeps for hard systems: after a Newton solve that needed at least
 * `switch_above` Krylov steps per Newton iteration the field split uses the alternative set, after
 * one that needed at most `back_below` the set of fedm_set_fieldsplit again (which also resets this).
 * A long polynomial pays while it saves whole Krylov steps: with the potential first in the split
 * (fedm_set_fieldsplit_order, opt-in) the species polynomial decides the Krylov count and the
 * alternative is a HIGHER degree; with the species first (default) the potential block limits the
 * convergence late in a run and the alternative is a cheaper one.  alt_sweeps = 0 switches the rule off. */
int fedm_set_fieldsplit_alternative(fedm_ctx *ctx, int alt_sweeps, const double *alt_weights,
                                    double switch_above, double back_below);
/* Which of the two sets ran: out = {policy (1: the set that is measured faster -- wall time per Newton iteration, one
 * GPU; 0: by the Krylov counts alone), alternative set active now, Newton solves run under the main set, under the
 * alternative set}.  The measured policy makes a run's trajectory of sets depend on the machine; bench.py prints
 * these counts per window so that two runs can be told apart (FEDM_FS_POLICY=counts: reproducible). */
int fedm_fieldsplit_policy(fedm_ctx *ctx, int64_t out[4]);
/* host-side greedy aggregation on a strength graph (set-up helper, no GPU needed) */
int fedm_amg_aggregate(int32_t n, const int64_t *indptr, const int32_t *indices,
                       const uint8_t *strong, int32_t *agg, int32_t *n_agg);

/* ---- multi-GPU (one process per GPU; what DOLFIN/PETSc do implicitly under mpirun,
 * README.md:63-67): ghost-value exchange before SpMV/assembly + all-reduces for dots/norms.
 * Plan in local vertex numbering: for neighbour k (rank nb_rank[k]) send the owned vertices
 * send_idx[send_ptr[k]..send_ptr[k+1]) and receive the ghost vertices
 * n_owned + [recv_ptr[k], recv_ptr[k+1]).  Both sides list a shared vertex set in the same
 * (global id) order. */
typedef void (*fedm_allreduce_fn)(double *host_buf, int32_t n, void *user);
typedef void (*fedm_exchange_fn)(const double *send_host, double *recv_host, int32_t width,
                                 void *user);
int fedm_comm_unique_id(void *out128 /* ncclUniqueId */);
int fedm_comm_init_rccl(fedm_ctx *ctx, int n_neighbours, const int32_t *nb_rank,
                        const int32_t *send_ptr, const int32_t *send_idx, const int32_t *recv_ptr,
                        const void *unique_id, int rank, int n_ranks);
/* host-staged transport owned by the caller (e.g. torch.distributed gloo); tests use it */
int fedm_comm_init_callbacks(fedm_ctx *ctx, int n_neighbours, const int32_t *nb_rank,
                             const int32_t *send_ptr, const int32_t *send_idx,
                             const int32_t *recv_ptr, fedm_allreduce_fn allreduce,
                             fedm_exchange_fn exchange, void *user, int rank, int n_ranks);
/* refresh the ghost entries of u_new, u_old, u_old1 from their owners */
int fedm_sync_ghosts(fedm_ctx *ctx);
/* Transport errors: every RCCL return code is checked; the first failure is latched in the
 * context (message in fedm_last_error), all later exchanges / reductions are skipped and
 * fedm_newton_solve, fedm_poisson_solve, fedm_sync_ghosts and fedm_field_error return -1.
 * fedm_comm_stats: out = {transport kind (0 none, 1 host callbacks, 2 RCCL), ranks, halo
 * exchanges issued, all-reduces issued, failed flag, neighbours, assembly patches without /
 * with ghost vertices (the former are assembled while the state halo travels), bytes this rank has
 * sent in halo exchanges, payload bytes it has contributed to all-reduces}. */
int fedm_comm_stats(fedm_ctx *ctx, int64_t out[10]);
/* latency of the transport's primitives, back to back on the compute stream (all ranks must call
 * it together): kind 0 = halo exchange of a block vector, 1 = of one value per vertex,
 * 2 = all-reduce of 32 doubles.  ms per operation. */
int fedm_time_comm(fedm_ctx *ctx, int kind, int repeats, double *ms_per_op);
/* Test hook (no GPU needed): drives the RCCL code path with a stub transport whose
 * `fail_at`-th call fails.  out = {failed flag latched, transport calls made, calls made after
 * the failing one, comm_failed(), ncclCommAbort calls at teardown, ncclCommDestroy calls at
 * teardown}: a failed communicator is aborted, never destroyed (its unfinished collective would
 * block ncclCommDestroy and every stream synchronisation after it).  Returns 1 when a failure was
 * latched. */
int fedm_debug_comm_fault(int fail_at, int64_t out[6]);
/* One halo exchange of the DOF vector `vec` (N values in the caller's order, ghost entries replaced by
 * what the neighbours sent) and one sum over the ranks of `red[0..k)`, through whatever transport the
 * context has: lets a test drive the transport's data path by itself (e.g. RCCL on one rank that is
 * its own neighbour).  The exchange runs twice (compute stream; communication stream fenced by events),
 * the sum twice (double; single-precision payload, so red comes back rounded to fp32).  red may be NULL. */
int fedm_debug_comm_roundtrip(fedm_ctx *ctx, double *vec, double *red, int k);
/* Host-side preprocessing alone (no GPU needed): what DOLFIN builds with the FunctionSpace /
 * sparsity pattern (fedm/functions.py:192,200).  out = {matrix slices (= assembly patches),
 * max cells per patch, max block columns per slice, max staged vertices per patch, cell visits
 * of all patches, owned (cell, local vertex) pairs, pairs that clash with another cell of their
 * 16-lane group on an LDS accumulator bank (FEDM_PATCH_ORDER, see csrc/prep.cpp), structural blocks,
 * stored blocks of the sliced block-ELL layout (structural + padding), halo vertices staged by all
 * patches, colours of the global cell colouring, (wave of 64 patch cells, local row) pairs in which some
 * cell owns that vertex: what the assembly kernels emit; the others are skipped}. */
int fedm_pattern_stats(const fedm_mesh_desc *mesh, int64_t out[12]);
/* The same for a live context, and which volume-assembly kernels its next fedm_jacobian call runs: out = {slices,
 * max cells per patch, max block columns per slice, max staged vertices per patch, cell visits, halo vertices,
 * assembly variant (0 global colouring, 1 LDS patches / unrolled element routine, 2 LDS patches / one
 * equation row at a time, 3 LDS patches / one pass over the cells), threads per workgroup, 1 when the one-pass
 * kernels run with the model's STRUCTURE compiled in (a precompiled signature matches it: csrc/assemble3.hip) and only
 * its numbers read at run time}.  The variant can change after the first Jacobian: that one writes all planes, the
 * later ones keep the constant planes and need less LDS. */
int fedm_pattern_info(fedm_ctx *ctx, int64_t out[9]);
/* The volume-assembly kernels the last residual-only assembly and the last Jacobian assembly actually launched:
 * out = {residual: variant (-1: none yet), threads per workgroup, launches, workgroups of all launches; Jacobian: the
 * same four}.  Variants 0..3 are fedm_pattern_info's (LFA family); the LMEA family's element kernels follow: 4
 * dual-number kernel per colour (FEDM_GD_HAND=0), 5 hand-derived blocks added with atomics (2, and the fall-back when
 * the element buffers cannot be allocated), 6 through the element buffer in cell order (4), 7 in the order of the
 * blocks' destinations (3), 8 the same with the three column vertices side by side (5); their gathers are not counted.
 * With several launches (the halo-overlap halves, the colouring's colours, FEDM_LEAN3_CLASSES) variant and threads are
 * the last one's. */
int fedm_launched_assembly(fedm_ctx *ctx, int64_t out[8]);
/* Which branches of the GMRES driver and of the Newton loop have run on this context since it was created (or since
 * the last call with reset != 0): host counters, nothing is added on the device.  out (may be NULL with reset) =
 *  [0] GMRES cycles that ran a Krylov step        [1] steps launched one by one, with their orthonormalising update
 *  [2] steps launched as part of a two-step graph  [3] steps launched 'as the last one' (without their update; singly
 *      or as the second step of a pair, which [2] then does not count)
 *  [4] steps launched ahead whose results were dropped (the solve ended before them, or a second Gram-Schmidt pass
 *      or a non-finite number made them void)       [5] skipped updates made up afterwards
 *  [6] second Gram-Schmidt passes                  [7] Newton updates fused with the GMRES update (<= 8 steps, one cycle)
 *  [8] generic updates delta += Z y (one per cycle otherwise)
 *  [9] solves with a deferred right-hand-side norm  [10] 'nothing to solve' exits
 *  [11] residual-only final checks of the Newton loop that were right   [12] ... that were wrong
 *  [13] fedm_field_error calls served from the cache
 *  [14] Krylov steps counted by the solves: [1] + [2] + [3] - [4]
 *  [15] steps launched before the step in front of them had been read   [16] ... in a cycle after the first
 *  [17] GMRES solves   [18] happy breakdowns   [19] solves stopped by ksp_max_it   [20] Newton solves stopped by max_it
 *  [21] true residuals formed at the start of a cycle: at every restart, and before a solve that ended on the generic
 *       update reports success   [22] ... that contradicted the recurrence's 'converged' (another cycle ran, or the
 *       solve gave up with FEDM_DIVERGED_LINEAR because such a cycle had not halved the residual)
 *  [23] second Gram-Schmidt passes that ran on the device, queued behind their step ([6] counts them too). */
int fedm_solver_path_stats(fedm_ctx *ctx, int64_t out[24], int reset);
/* Test hook: x = the GMRES solution of J x = b with the Jacobian and the preconditioner as the last fedm_jacobian /
 * fedm_newton_solve left them, through the very call fedm_newton_solve makes (same preparation of the preconditioner
 * and of the right-hand side for the side in use; opts' ksp_* fields are read).  The state is not touched; F of the
 * last assembly is overwritten with -b.  b and x in the caller-side layout of fedm_residual.  Returns what the solver
 * returns (0, FEDM_DIVERGED_LINEAR, FEDM_DIVERGED_NAN); its / rnorm: its step count and the residual norm it reports
 * (on the left: of the preconditioned residual M^-1 r; on the right: of the true residual, |b - J x|_2 -- and with
 * fedm_set_krylov_scaling "rows" the row-equilibrated |D (b - J x)|_2, tested against max(ksp_rtol |D b|_2, ksp_atol)). */
int fedm_debug_linear_solve(fedm_ctx *ctx, const double *b, const fedm_newton_opts *opts, double *x, int *its,
                            double *rnorm);
/* F as the last assembly left it (residual-only or F + J: no evaluation), caller-side layout as fedm_residual's. */
int fedm_get_residual(fedm_ctx *ctx, double *F_out);
/* The species sweeps of the field split (the Chebyshev polynomial in Duu^-1 Juu that stands for PETSc's
 * sub-solver of the species block; no counterpart in the scripts): on one GPU they run several per launch on
 * tiles of matrix slices whose vertex layers sit in LDS (csrc/fs_tiles.hip).  Returns 1 when this context
 * does so (builds the tiles if need be), 0 when it runs them one by one (several GPUs, more than two species,
 * FEDM_FS_TILES=0); out = {tiles, slices per tile, vertex layers (= sweeps per launch), longest matrix row,
 * most vertices of a tile with its layers, most rows, bytes of the tile tables, threads per tile, rows of all
 * tiles (the tile's own and the layers': the redundancy is this over the vertex count), vertices of all tiles}. */
int fedm_fieldsplit_tiles_info(fedm_ctx *ctx, int64_t out[10]);
/* The tile tables of a mesh built on the host alone (no GPU needed), with a self-check: out = {tiles, longest
 * matrix row, most vertices of a tile with its layers, most rows, rows of all tiles, vertices of all tiles, bytes,
 * violations found (0: every vertex is the own vertex of exactly one tile, the layers nest, every local column
 * number names the vertex the block pattern names), dynamic LDS bytes per workgroup of the species-sweep kernel
 * (two species) and of the multigrid-sweep kernel on these tiles: tiles whose kernels would need more than the
 * device grants a workgroup (160 KiB on gfx950) are refused when a context builds them}. */
int fedm_fieldsplit_tiles_stats(const fedm_mesh_desc *mesh, int tile_slices, int depth, int64_t out[10]);
/* Test hook: z = Minv t with the field-split preconditioner of the CURRENT Jacobian (fedm_jacobian first; its
 * species planes are formed here), host vectors of n_vertices * n_eq doubles -- the operator a Krylov step of
 * fedm_newton_solve applies, alone. */
int fedm_debug_fieldsplit_apply(fedm_ctx *ctx, const double *t, double *z);
/* Test hook: t = J v and z = Minv t as a Krylov step of the LEFT-preconditioned GMRES forms them (the operator
 * Minv J, fedm_set_preconditioner_side "left") -- the Jacobian product with the field split's first stage in its
 * epilogue, then the rest of the preconditioner (lower-triangular order only); host vectors as in
 * fedm_debug_fieldsplit_apply. */
int fedm_debug_fieldsplit_apply_operator(fedm_ctx *ctx, const double *v, double *t, double *z);
/* Test hook: z = Minv y as a Krylov step of the RIGHT-preconditioned GMRES forms it on one GPU with species sweeps
 * (FEDM_FS_FIRST_BY_PRODUCER): the kernel that completes the Krylov vector y also forms the preconditioner's first
 * stage, the preconditioner skips its own.  k = 0: y = coef[0] t (the vector scaling); k = 1..8: y = (t - sum_i
 * coef[i] t) coef[k] (the Gram-Schmidt update over k basis vectors, all of them t).  y and z are returned (host
 * vectors as in fedm_debug_fieldsplit_apply). */
int fedm_debug_fieldsplit_apply_produced(fedm_ctx *ctx, const double *t, int k, const double *coef, double *y,
                                         double *z);
/* Test hook: mode 0 = species sweeps one launch each from now on (and the multigrid's finest-level sweeps kernels of
 * their own); 3 = species sweeps on tiles, the multigrid's not; 1 = tiles, rebuilt with `tile_slices` slices
 * per tile, `depth` vertex layers and `threads` threads per tile (0: defaults, FEDM_FS_TILE_SLICES /
 * FEDM_FS_TILE_DEPTH / FEDM_FS_TILE_THREADS). */
int fedm_debug_fieldsplit_tiles(fedm_ctx *ctx, int mode, int tile_slices, int depth, int threads);
/* Test hook: the field split's species planes as they stand (formed by the one-pass assembly itself plus the rows
 * changed behind it, or by the separate pass) against the separate pass over the Jacobian as it stands.
 * out[4] = {max |d Duu^-1| / max |Duu^-1|, max |d S16|, max |d coupling| / max |coupling|, 1 if the last set-up was
 * the fused one}. */
int fedm_debug_species_planes_check(fedm_ctx *ctx, double *out);

/* Test hook: ONE launch wrapper of a Krylov step's reductions and vector updates (csrc/kernels.hip, the second half of
 * csrc/spmv.hip) on the caller's vectors -- the production wrapper itself, with the production grids.
 *   Vectors are host arrays of n_vertices * n_eq doubles in the device's order (fedm_debug_fieldsplit_apply's).  They
 * go into the Krylov storage (ensure_krylov(30): V[i] for i < 31, the first preconditioned vector for i = 31), y into
 * the product vector, x into the scratch vector.  Every device entry outside the part of a vector that takes part in
 * reductions is overwritten with `sentinel` (finite): the padding rows [n, np) and, with n_owned < n_vertices, the
 * ghost rows -- a kernel that reads a wrong range shows it.  Exceptions, because the entries are operands: x of
 * FEDM_KOP_SPMV_DOTS keeps the caller's ghost entries, and x0 (n_vertices doubles) is sentinel beyond n_vertices only.
 *   red[2][FEDM_KOP_RED_K]: the reductions' result rows; uploaded first when red_in is set (coefficients live there),
 * zero otherwise; always returned.  mail[FEDM_KOP_RED_K]: the mailbox slot of the op's last publication, when it made
 * one.  info = {publications made, host count of publications, device count (the two must agree; -1 when the entry
 * found them apart), 1 if the Krylov storage was allocated by this call}.  With fedm_set_krylov_scaling "rows" the
 * reductions take their weighted instantiations with the weights of the Jacobian as it stands.
 *   The context is left as found (state, reduction rows, scaling); only scratch vectors are overwritten.
 * op, k and the fields read:
 *   DOTS             red[i] = V[i] . y, i < k <= 32; finish: the finish formulae on them and a publication
 *   DOTS_FUSED       the same through dots_scatter_kernel; y_index >= 0: y IS V[y_index] (and y is not read from the
 *                    caller); x0: the potential component of y is taken from it first; y_out returns y
 *   SPMV_DOTS        y = J x, red[i] = V[i] . y (i < k - 1), red[k-1] = y . y; 2 <= k <= 8, three equations; finish 0,
 *                    1, 2 (SPMV_DOTS_SUMS, _PUBLISH, _REFINED)
 *   CGS_REFINE       the second Gram-Schmidt pass behind step j = k - 2 on y with V[0 .. j]; red_in carries the flag
 *   NORM2            red[slot] = y . y;   NORM2_PUBLISH  the same and the publication of red[0 .. k)
 *   CGS_UPDATE       y = (y - sum_i red[i] V[i]) red[RED_K-1], k <= 32
 *   CGS_UPDATE_FS    the same for k <= 4 with the field split's first stage: g32 [n_vertices][2] and b0 [n_vertices]
 *   SCALE_COPY_FS    y = a x with that first stage
 *   MULTI_AXPY       y += a sum_i coef[i] V[i], k <= 32
 *   NEWTON_UPDATE    delta = sum_i coef[i] V[i], y += delta, red[1] = |delta|^2, red[2] = |y|^2, k <= 8; finish = 0:
 *                    delta is not stored; x_out returns delta
 *   NORMALISE_COPY   y = x / sqrt(red[slot])
 *   FIELD_ERROR(_SLOTS34)  component `slot` of y against x as new and old state: red[0..1] (red[3..4])
 * Refused (-2, nothing launched): k out of the op's range or beyond n_vec, SPMV_DOTS on a model without exactly three
 * equations, an _FS op or CGS_REFINE without two species and the field split's buffers (fedm_amg_setup,
 * fedm_set_fieldsplit with more than one sweep), a missing vector. */
#define FEDM_KOP_RED_K 40
#define FEDM_KOP_MAX_VECTORS 32
enum {
    FEDM_KOP_DOTS = 0, FEDM_KOP_DOTS_FUSED, FEDM_KOP_SPMV_DOTS, FEDM_KOP_CGS_REFINE, FEDM_KOP_NORM2,
    FEDM_KOP_NORM2_PUBLISH, FEDM_KOP_CGS_UPDATE, FEDM_KOP_CGS_UPDATE_FS, FEDM_KOP_SCALE_COPY_FS, FEDM_KOP_MULTI_AXPY,
    FEDM_KOP_NEWTON_UPDATE, FEDM_KOP_NORMALISE_COPY, FEDM_KOP_FIELD_ERROR, FEDM_KOP_FIELD_ERROR_SLOTS34,
    FEDM_KOP_COUNT
};
typedef struct {
    int32_t n_vec;        /* vectors in V                                                   */
    int32_t finish;       /* DOTS, DOTS_FUSED: 0 / 1; SPMV_DOTS: 0 / 1 / 2; NEWTON_UPDATE: store delta */
    int32_t y_index;      /* DOTS_FUSED: y is V[y_index]; -1: a vector of its own           */
    int32_t slot;         /* NORM2, NORM2_PUBLISH, NORMALISE_COPY; FIELD_ERROR*: component  */
    int32_t red_in;       /* upload red before the op                                       */
    int32_t pad_;
    double a;             /* SCALE_COPY_FS: factor; MULTI_AXPY: sign                        */
    double sentinel;
    const double *V;      /* [n_vec][n]                                                     */
    const double *y;      /* [n]                                                            */
    const double *x;      /* [n]                                                            */
    const double *x0;     /* [n_vertices] or null                                           */
    const double *coef;   /* [k] host coefficients (MULTI_AXPY, NEWTON_UPDATE)              */
    double *red;          /* [2][FEDM_KOP_RED_K], in / out                                  */
    double *y_out;        /* [n] or null                                                    */
    double *x_out;        /* [n] or null                                                    */
    double *mail;         /* [FEDM_KOP_RED_K] or null                                       */
    float *g32;           /* [n_vertices][2] or null                                        */
    double *b0;           /* [n_vertices] or null                                           */
    int64_t info[4];
} fedm_krylov_io;
int fedm_debug_krylov_op(fedm_ctx *ctx, int op, int k, fedm_krylov_io *io);

/* |new - old + eps| / |old + eps| on one component        fedm/functions.py:1062-1064 */
int fedm_field_error(fedm_ctx *ctx, int component, double *rel_err);

/* ---- discharge diagnostics on the device ------------------------------------------------------
 * What a streamer run reports per step (Bagheri et al. 2018: head position, maximal field, particle numbers) and the
 * integrated form of BoundaryGradient (fedm/functions.py), from the resident state in one pass over the cells and one
 * over the vertices; one small read-back per call.  LFA family (fedm_ctx_create, _tabulated, _walls; with or without
 * photoionisation); densities n_s = exp(u_s), or u_s with linear_representation.  Throughout
 *     W_q = qp_w[q] |det J| 2 pi w(x_q),   w = r (axisymmetric) or 1/(2 pi),
 * the weight of the residual, at the model's own quadrature points; |E|, mu_s and D_s once per cell, as the element
 * routines have them.  Every sum and maximum is reduced in a fixed order without floating-point atomics: two calls on
 * the same state return the same bytes.
 * Several ranks (n_owned_vertices < n_vertices): every quadrature term of an integral is multiplied by
 * sum_(a owned) phi_a(x_q), so the ranks' shares add up to the global integral; group sums run over owned group
 * vertices, field maxima over the cells with an owned vertex, nodal maxima over the owned vertices.  The call makes no
 * reduction over the ranks.  On one GPU the factor is exactly 1. */
#define FEDM_DIAG_MAX_GROUPS 8
typedef struct {
    int32_t state;                /* 0: u_new, 1: u_old                                                          */
    int32_t pad_;
    double r_lo, r_hi, z_lo, z_hi; /* closed window [r_lo, r_hi] x [z_lo, z_hi] of cell centroids [m]; -inf / +inf
                                      bounds make it the whole mesh                                              */
} fedm_diag_opts;
typedef struct {
    /* N_s = sum_cells sum_q W_q n_s(x_q): particles (axisymmetric) or particles per metre of depth (planar)      */
    double species_integral[FEDM_MAX_SPECIES];
    /* q_g = sum_(i in group g + 1) R_Phi,i with the unconstrained Poisson row
     *   R_Phi,i = sum_cells sum_q W_q (grad Phi . grad phi_i - (e/eps0) sum_s Z_s n_s phi_i)   [V m; V planar]:
     * eps0 q_g is the charge on the electrode [C; C/m planar]                                                    */
    double group_sum[FEDM_DIAG_MAX_GROUPS];
    /* I_psi = sum_s Z_s sum_cells sum_q W_q Gamma_s(x_q) . (-grad psi)  [1/s; 1/(s m) planar], Shockley-Ramo with the
     * residual's own flux: Gamma_s = n_s (-D_s grad u_s + Z_s mu_s E), linear representation -D_s grad u_s +
     * Z_s mu_s E u_s; drift_w in place of Z mu E where has_drift_w; 0 for 'reaction' species, and without a psi.
     * e I_psi is the current [A]                                                                                 */
    double induced_current;
    /* max over the cells of |E| = |grad Phi| [V/m], its cell (the caller's index; lowest on a tie) and that cell's
     * centroid (x_0 + x_1 + x_2)/3 [m]; 0 and -1 without a Poisson equation                                      */
    double field_max, field_max_centroid[2];
    /* the same over the cells whose centroid lies in the window; 0 and -1 when there is none                     */
    double window_max, window_max_centroid[2];
    /* max_v u_s(v), bitwise a value of the state (exp is the caller's), and its vertex in the CONTEXT's numbering
     * (lowest on a tie; -1 when the rank owns no vertex)                                                         */
    double nodal_max[FEDM_MAX_SPECIES];
    int32_t field_max_cell, window_max_cell;
    int32_t nodal_max_vertex[FEDM_MAX_SPECIES];
    /* 0: a state value visited or a cell quantity formed was not finite; the other fields are then unspecified   */
    int32_t finite;
    int32_t pad_;
} fedm_diag;
/* psi: nodal P1 weighting potential [n_vertices] (dimensionless, 1 on the electrode whose current is asked for) or NULL;
 * group: [n_vertices] values 0 (none) or 1..n_groups, or NULL with n_groups = 0; both in the context's numbering, copied.
 * Replaces an earlier set-up.  Refused (-2, fedm_last_error says why): an LMEA context; n_groups outside
 * 0..FEDM_DIAG_MAX_GROUPS or without an array; a group value outside 0..n_groups; groups in a model without a Poisson
 * equation; a psi that is not finite. */
int fedm_diag_setup(fedm_ctx *ctx, const double *psi, const int8_t *group, int n_groups);
/* The quantities above of the chosen state; works without fedm_diag_setup (no psi, no groups).  The state is not
 * touched.  Returns 0 also when out->finite is 0; the next call is unaffected.  Refused (-2): an LMEA context, a null
 * argument, a state selector other than 0 or 1, a window bound that is NaN. */
int fedm_diagnostics(fedm_ctx *ctx, const fedm_diag_opts *opts, fedm_diag *out);

/* ---- field output on the device ---------------------------------------------------------------
 * Derived nodal fields and point probes from the resident state, blended in time the way file_output blends
 * (fedm/file_io.py:538-616), without downloading the state.  LFA family (fedm_ctx_create, _tabulated, _walls; with or
 * without photoionisation), logarithmic or linear representation.  Kinds, in the caller's units:
 *   STATE    index = equation e   u_e(v): a value of the state, no arithmetic but the blend
 *   DENSITY  index = species s    exp(u_s(v)), or u_s(v) with linear_representation
 *   CHARGE   -                    e sum_s Z_s n_s(v), e = FEDM_ELEMENTARY_CHARGE, species in ascending order
 *   E_R, E_Z -                    the cell-constant -dPhi/dr, -dPhi/dz, projected
 *   E_NORM   -                    the cell-constant |E| = |grad Phi|, projected
 *   RATE     index = reaction j   R_j = k_j(|E|) prod_i n_i^p_ji, k_j once per cell, the densities at the quadrature
 *                                 points (the source photoionisation integrates), projected
 *   FLUX_R, FLUX_Z  index = species s   the residual's own flux n_s (-D_s grad u_s + Z_s mu_s E), linear
 *                                 representation -D_s grad u_s + Z_s mu_s E u_s; drift_w in place of Z mu E where
 *                                 has_drift_w; 0 for 'reaction' species (what fedm_diagnostics integrates), projected
 * The first three are pointwise.  Projection uses the plain measure dx (no r weight, no 2 pi; DOLFIN's project):
 *   b_v = sum_(c with v) sum_q qp_w[q] |det J_c| f(x_q) phi_v(x_q)   at the model's own quadrature points,
 *   m_v = sum_(c with v) |det J_c| / 6,
 *   lumped X_v = b_v / m_v;  consistent: M X = b with the P1 mass matrix of fedm_fields_setup, conjugate gradients with
 *   Jacobi from X = 0 until the recurrence's |r|_2 <= rtol |b|_2.
 * b_v and m_v add their cells' entries in ascending (cell, corner) order and nothing adds with floating-point atomics:
 * two calls on one state return the same bytes.  Without a Poisson equation the coefficients are taken at |E| = 1, as
 * the element routines take them.
 * Several ranks (n_owned_vertices < n_vertices): every cell of an owned vertex is local, so pointwise kinds and the
 * lumped projection are exact on the owned vertices without communication; ghost entries are written as 0.  The
 * consistent projection and probes are refused there. */
#define FEDM_FIELD_STATE 0
#define FEDM_FIELD_DENSITY 1
#define FEDM_FIELD_CHARGE 2
#define FEDM_FIELD_E_R 3
#define FEDM_FIELD_E_Z 4
#define FEDM_FIELD_E_NORM 5
#define FEDM_FIELD_RATE 6
#define FEDM_FIELD_FLUX_R 7
#define FEDM_FIELD_FLUX_Z 8
#define FEDM_FIELDS_MAX_REQ 8
#define FEDM_ELEMENTARY_CHARGE 1.6021766208e-19   /* fedm/physical_constants.py:5 */
typedef struct {
    int32_t kind, index;
} fedm_field_req;
typedef struct {
    double num, den;      /* out = X(u_old) + num * (X(u_new) - X(u_old)) / den, the expression of file_output (num =
                             t_out - t_old, den = t - t_old), rounded operation by operation; num == den: X(u_new)
                             alone, num == 0: X(u_old) alone (one evaluation, no arithmetic)                      */
    int32_t projection;   /* 0 lumped, 1 consistent                                                                */
    int32_t max_it;       /* conjugate-gradient steps at the most (consistent)                                     */
    double rtol;
} fedm_field_opts;
/* Once per context; replaces an earlier set-up (and drops its probes).  mass: the P1 mass matrix of the plain measure
 * in the context's numbering, n_vertices x n_vertices, copied; NULL: lumped projection only.  Allocates every buffer
 * fedm_fields uses.  Refused (-2): an LMEA context; a mass matrix of another size, or on a context with ghosts. */
int fedm_fields_setup(fedm_ctx *ctx, const fedm_csr *mass);
/* n_points points, each three vertices of the context's numbering and three weights: probe = sum_a w_a X[v_a], added
 * in that order.  Replaces earlier points; n_points = 0 drops them.  Refused (-2): before fedm_fields_setup; a context
 * with ghosts; a vertex out of range; a weight that is not finite. */
int fedm_probe_setup(fedm_ctx *ctx, int n_points, const int32_t *vertices, const double *weights);
/* n_req <= FEDM_FIELDS_MAX_REQ fields of the resident state.  nodal: [n_req][n_vertices] in the context's numbering, or
 * NULL; probes: [n_req][n_points], or NULL (with nodal NULL only n_req * n_points doubles come back); finite: 0 when a
 * state value of an owned vertex or a result was not finite (the call still returns 0, the next call is unaffected);
 * cg_iterations: [n_req] or NULL, 0 for requests without a solve.  Allocates nothing; the lumped and pointwise kinds
 * synchronise once, for the read-back (a consistent projection reads its reductions as it goes).
 * Returns FEDM_DIVERGED_LINEAR when a consistent projection stopped at max_it.  Refused (-2, fedm_last_error names the
 * cause): before fedm_fields_setup; an LMEA context; n_req outside 1..FEDM_FIELDS_MAX_REQ; an unknown kind; an index out
 * of range; E_R, E_Z, E_NORM without a Poisson equation, and FLUX_* of a drift-diffusion species without drift_w there
 * (a species with drift_w, or a diffusion-reaction species, has its flux as fedm_diagnostics has it); projection other
 * than 0 or 1, 1 without a mass matrix or with ghosts, 1 with max_it < 1 or rtol <= 0; den == 0; a num, den or rtol that
 * is not finite; probes asked for without points. */
int fedm_fields(fedm_ctx *ctx, const fedm_field_opts *opts, int n_req, const fedm_field_req *req, double *nodal,
                double *probes, int32_t *finite, int32_t *cg_iterations);

/* ---- field output of LMEA models on the device ------------------------------------------------
 * The same for the LMEA family (fedm_ctx_create_gd), one GPU: where things happen in a glow discharge, without
 * downloading the states and the field table.  fedm_field_req, fedm_field_opts, FEDM_FIELDS_MAX_REQ, the meaning of num,
 * den, projection, max_it and rtol, the result layout, the finite flag and the return codes are fedm_fields'.  Notation
 * is the balance's: ns = n_species; component c = 0 is the energy, c = 1..ns-1 the species (ns-1 the electrons), ns the
 * potential; species index 0 is the gas.  Kinds (numbers of their own; an LFA kind is an unknown kind here):
 *  pointwise, from a state alone (may be blended):
 *   STATE    index = equation e   u_e(v), bitwise
 *   DENSITY  index = component c  exp(u_c(v)); c = 0: the energy density
 *   CHARGE   -                    e sum_(s >= 1) sign_s exp(u_s(v)), in ascending order
 *   MEAN_ENERGY -                 exp(u_0(v) - u_e(v)), as fedm_gd_update_mean_energy forms it
 *  pointwise, from the field table:
 *   TABLE    index = row f        row f of fedm_gd_set_fields as it stands, bitwise
 *  projected, from the potential alone (may be blended):
 *   E_R, E_Z, E_NORM -            the cell-constant -dPhi/dr, -dPhi/dz, |grad Phi|
 *   REDUCED_FIELD -               1e21 |grad Phi| / N0, the reference's redE (fedm-gd.py:432)
 *  projected, as the residual of the current step evaluates it -- u_new, the field table as it stands, the
 *  semi-implicit coefficients c + c' dme at the quadrature points (fedm_gd_balance's notation):
 *   RATE     index = reaction j   R_j = k_j N0^p_j0 prod_i n_i^p_ji, multiplied in the residual's order
 *   SOURCE   index = species s >= 1   sum_j net[j][s] R_j, reactions in ascending order
 *   COLLISION_LOSS -              sum_j loss_j R_j, the two sentinel losses as the residual takes them
 *   JOULE    -                    -Gamma_e . E
 *   FLUX_R, FLUX_Z  index = component c   c >= 1: the flux of the species' row: 0 for 'reaction',
 *                                 -grad(D n) for 'diffusion-reaction', the drift-diffusion flux otherwise; c = 0: the
 *                                 energy row's flux, the electrons' with 5/3 D_e, 5/3 mu_e on u_0
 *   CURRENT_R, CURRENT_Z -        e sum_(s >= 1) sign_s Gamma_s, the conduction current density
 * The kinds of the last group and TABLE have no state selector, for the balance's reason (the table belongs to the
 * current step): a call that contains one needs num == den.  Called after an accepted step and before the next
 * fedm_gd_prep_step they are the fields of the step just solved.
 * Projection is fedm_fields': the plain measure qp_w |det J| at the model's own quadrature points, b_v and m_v added in
 * ascending (cell, corner) order, no floating-point atomics, lumped or consistent with the mass matrix of the set-up.
 * Two calls on one state return the same bytes; a call touches no state and no table row. */
#define FEDM_GD_FIELD_STATE 32
#define FEDM_GD_FIELD_DENSITY 33
#define FEDM_GD_FIELD_CHARGE 34
#define FEDM_GD_FIELD_MEAN_ENERGY 35
#define FEDM_GD_FIELD_TABLE 36
#define FEDM_GD_FIELD_E_R 37
#define FEDM_GD_FIELD_E_Z 38
#define FEDM_GD_FIELD_E_NORM 39
#define FEDM_GD_FIELD_REDUCED_FIELD 40
#define FEDM_GD_FIELD_RATE 41
#define FEDM_GD_FIELD_SOURCE 42
#define FEDM_GD_FIELD_COLLISION_LOSS 43
#define FEDM_GD_FIELD_JOULE 44
#define FEDM_GD_FIELD_FLUX_R 45
#define FEDM_GD_FIELD_FLUX_Z 46
#define FEDM_GD_FIELD_CURRENT_R 47
#define FEDM_GD_FIELD_CURRENT_Z 48
/* fedm_fields_setup and fedm_probe_setup for an LMEA context.  Refused (-2, fedm_last_error names the cause): an LFA
 * context; a context with ghosts; what fedm_fields_setup / fedm_probe_setup refuse for the same arguments. */
int fedm_gd_fields_setup(fedm_ctx *ctx, const fedm_csr *mass);
int fedm_gd_probe_setup(fedm_ctx *ctx, int n_points, const int32_t *vertices, const double *weights);
/* fedm_fields for an LMEA context, with the kinds above.  Refused (-2): an LFA context; a context with ghosts; before
 * fedm_gd_fields_setup; n_req outside 1..FEDM_FIELDS_MAX_REQ; an unknown kind; an index out of range (SOURCE: 1..ns-1);
 * a residual-evaluated kind or TABLE with num != den (the message names the request); projection other than 0 or 1, 1
 * without a mass matrix, 1 with max_it < 1 or rtol <= 0; den == 0; a num, den or rtol that is not finite; probes asked
 * for without points.  A refused call leaves the next one unaffected. */
int fedm_gd_fields(fedm_ctx *ctx, const fedm_field_opts *opts, int n_req, const fedm_field_req *req, double *nodal,
                   double *probes, int32_t *finite, int32_t *cg_iterations);

/* ---- particle and energy balance of LMEA models on the device ------------------------------------
 * What a glow-discharge run is judged by, from the resident state in one pass over the cells, one over the tagged
 * boundary facets and one over the vertices; one small read-back per call.  LMEA family (fedm_ctx_create_gd), one GPU.
 * Notation: ns = n_species; component c = 0 is the energy equation, c = 1..ns-1 the species (ns-1 the electrons), ns
 * the potential.  W = qp_w |det J| 2 pi r(x_q) at the model's own quadrature points, 1/(2 pi) in place of r when
 * axisymmetric == 0; on a facet W = fqp_w L 2 pi r.  Everything is evaluated at u_new with the field table as it
 * stands and the context's u_old, u_old1, dt, dt_old: exactly what the residual of the current step sees -- the
 * semi-implicit coefficients c + c' dme, dme = (exp(u_0) - exp(u_e) mean_energy_old) / exp(u_e_old), the fluxes
 * Gamma_s of the species rows, the facet integrands of the 'flux source' walls.  There is no state selector: called
 * after an accepted step and before the next fedm_gd_prep_step it is the balance of the step just solved.
 * The P1 basis sums to 1 and its gradient to 0, and species and energy rows carry no Dirichlet condition, so the sum
 * over ALL vertices of row c of the assembled residual is, in exact arithmetic,
 *     rate_of_change[c] - source[c] + sum_t wall[t][c],
 * with the sources the caller forms: source[s] = sum_j net[j][s] reaction[j], source[0] = joule - collision_loss.
 * Every sum and maximum is reduced in a fixed order without floating-point atomics: two calls on one state return the
 * same bytes. */
#define FEDM_GD_BAL_MAX_GROUPS 8
/* (a struct tag, not a typedef: the call below has the same name, so the type is written `struct fedm_gd_balance`) */
struct fedm_gd_balance {
    double content[FEDM_GD_MAX_SPECIES];        /* sum W exp(u_c): particles; c = 0 the electrons' energy [eV]            */
    double rate_of_change[FEDM_GD_MAX_SPECIES]; /* sum W T_c, T_c = exp(u_c) ((1 + 2w) u_c - (1 + w)^2 u_c,old +
                                                   w^2 u_c,old1) / ((1 + w) dt), w = dt / dt_old: the residual's BDF2 term */
    double reaction[FEDM_GD_MAX_REACTIONS];     /* sum W R_j, R_j = k_j N0^p_j0 prod_i n_i^p_ji with the semi-implicit k_j,
                                                   multiplied in the residual's order                                   */
    double collision_loss, joule;               /* sum W sum_j loss_j R_j (the two sentinel losses as the residual takes
                                                   them); sum W (-Gamma_e . E)   [eV/s]                                  */
    double wall[FEDM_MAX_TAGS][FEDM_GD_MAX_SPECIES]; /* the facet integrand of row c summed over the facets with tag t + 1:
                                                   (1 - ref)/(1 + ref) (vth/2 + |sign mu E.n|) n - 2 gamma/(1 + ref) ion
                                                   flux for electrons; 5/3 mu, 1.3333 vth, gamma we_secondary for c = 0;
                                                   0 for 'reaction' species                                             */
    double ion_flux[FEDM_MAX_TAGS];             /* sum W sum_ions max(Gamma_i . n, 0)                                    */
    double induced_current;                     /* sum_(s >= 1) sign_s sum W Gamma_s . (-grad psi) [1/s], the residual's
                                                   fluxes; 0 without a psi                                              */
    double group_sum[FEDM_GD_BAL_MAX_GROUPS];   /* the unconstrained Poisson rows summed over the group's vertices, as
                                                   fedm_diag.group_sum                                                  */
    double field_max, field_max_centroid[2];    /* max over the cells of |grad Phi|, its cell (the context's cell index, lowest
                                                   on a tie), that cell's centroid                                      */
    double nodal_max[FEDM_GD_MAX_SPECIES + 1];  /* c < ns: max_v u_c(v), bitwise a state value; [ns]: max_v (u_0 - u_e)(v),
                                                   the log of the mean energy                                           */
    int32_t field_max_cell, nodal_max_vertex[FEDM_GD_MAX_SPECIES + 1];   /* lowest on a tie; -1 for unused entries       */
    int32_t finite, pad_;                       /* 0: a state value visited or a quantity formed was not finite; the
                                                   other fields are then unspecified                                    */
};
/* psi: nodal P1 weighting potential [n_vertices] or NULL; group: [n_vertices] values 0 (none) or 1..n_groups, or NULL
 * with n_groups = 0; both in the context's numbering, copied.  Replaces an earlier set-up.  Refused (-2, fedm_last_error
 * says why): an LFA context; a context with ghosts; n_groups outside 0..FEDM_GD_BAL_MAX_GROUPS or without an array; a
 * group value outside 0..n_groups; a psi that is not finite. */
int fedm_gd_balance_setup(fedm_ctx *ctx, const double *psi, const int8_t *group, int n_groups);
/* The quantities above; works without fedm_gd_balance_setup (no psi, no groups).  Allocates nothing after the first
 * call, touches no state and synchronises once, for the read-back.  Returns 0 also when out->finite is 0; the next
 * call is unaffected.  Refused (-2): an LFA context, a context with ghosts, a null argument. */
int fedm_gd_balance(fedm_ctx *ctx, struct fedm_gd_balance *out);

/* ---- electrode currents (both families; models with a Poisson equation; one GPU) ------------------------------------
 * Shockley-Ramo currents of up to FEDM_CURRENTS_MAX weighting potentials psi_g at once, from the resident state.
 * W is the residual's weight, qp_w |det J| 2 pi w(x_q) with w = r (axisymmetric) or 1/(2 pi) (planar), at the model's
 * own quadrature points -- what fedm_diagnostics and fedm_gd_balance document.
 *   conduction: fedm_diag.induced_current (LFA: the fluxes of fedm_diagnostics at u_new; log and linear representation,
 *     drift_w, 0 for 'reaction' species, tables) or fedm_gd_balance.induced_current (LMEA: the residual's own fluxes of
 *     the current step, species s >= 1 with sign_s) for each psi_g.
 *   D_t Phi: the variable-step BDF2 quotient of the species rows' time term,
 *     ((1 + 2w) Phi - (1 + w)^2 Phi_old + w^2 Phi_old1) / ((1 + w) dt),  w = dt / dt_old,
 *     from the potential entries of u_new, u_old, u_old1, nodal; its gradient per cell.
 *   With E = -grad Phi and E_w = -grad psi,  eps0 d_t E . E_w = eps0 grad(d_t Phi) . grad psi:
 *   e conduction + eps0 displacement is the total current with the sign induced_current has.
 *   capacitance: formed in fedm_currents_setup and after fedm_currents_solve, [g][h] and [h][g] from one sum.
 * Every sum is reduced in a fixed order without floating-point atomics: two calls on one state return the same bytes. */
#define FEDM_CURRENTS_MAX 8
/* (a struct tag, not a typedef: the call below has the same name, so the type is written `struct fedm_currents`) */
struct fedm_currents {
    double conduction[FEDM_CURRENTS_MAX];      /* sum_s Z_s sum W Gamma_s . (-grad psi_g)        [1/s]    */
    double displacement[FEDM_CURRENTS_MAX];    /* sum W grad(D_t Phi) . grad psi_g               [V m/s]  */
    double coupling[FEDM_CURRENTS_MAX];        /* sum W grad Phi(u_new) . grad psi_g             [V m]    */
    double induced_charge[FEDM_CURRENTS_MAX];  /* sum_s Z_s sum W n_s psi_g                      [1]      */
    double capacitance[FEDM_CURRENTS_MAX][FEDM_CURRENTS_MAX];   /* sum W grad psi_g . grad psi_h  [m]      */
    int32_t n_psi, finite;                     /* finite 0: a state value visited or a quantity formed was not finite;
                                                  the sums are then unspecified                                         */
};
/* psi: n_psi nodal P1 weighting potentials [n_psi][n_vertices] in the context's numbering, copied; the capacitance
 * matrix is formed.  Replaces an earlier set-up.  Refused (-2, fedm_last_error says why): no Poisson equation; a context
 * with ghost vertices or a transport; n_psi outside 1..FEDM_CURRENTS_MAX; a null argument; a psi that is not finite. */
int fedm_currents_setup(fedm_ctx *ctx, int n_psi, const double *psi);
/* Solves for the installed potentials on the device.  laplace->A[0] is K_w (int w grad phi_a . grad phi_b) in the
 * context's numbering with rows and columns of the conductors' (Dirichlet) vertices eliminated symmetrically: those
 * vertices are the unit rows of A[0], and the installed psi_g carries their values.  Per potential, conjugate gradients
 * preconditioned by the hierarchy (n_levels = 1: Jacobi), as fedm_photo_setup takes it, for the free vertices' values
 * with rhs_g (-K_w psi_D on the free rows; the unit rows' entries are not read) until |r|_2 <= rtol |rhs|_2 on the
 * recurrence's residual; the conductors' values stay bitwise.  The capacitance is formed again.  iterations (unless
 * NULL): CG steps per potential.  Returns 0, FEDM_DIVERGED_LINEAR (a potential stopped at max_it) or FEDM_DIVERGED_NAN
 * (an operator that is not positive definite, a NaN on the way); a failed solve leaves every installed potential and the
 * capacitance as they were.  Refused (-2): the refusals of fedm_currents_setup; no set-up; an rhs that is not finite;
 * rtol <= 0 or max_it < 0; a hierarchy that fedm_amg_setup would refuse or whose operator is not n_vertices square. */
int fedm_currents_solve(fedm_ctx *ctx, const fedm_photo_hierarchy *laplace, const double *rhs, double rtol, int max_it,
                        int iterations[FEDM_CURRENTS_MAX]);
/* Test hook: the installed potentials [n_psi][n_vertices], the context's numbering. */
int fedm_currents_get_psi(fedm_ctx *ctx, double *psi);
/* One pass over the cells, a one-workgroup finish, one read-back.  Touches no state and no field table; returns 0 also
 * when out->finite is 0, and the next call is unaffected.  Refused (-2): as fedm_currents_setup; no set-up. */
int fedm_currents(fedm_ctx *ctx, struct fedm_currents *out);

/* ---- external circuit of the driven electrodes (both families; what the electrode currents need; one GPU) -------------
 * The n conductors of the fedm_currents_setup in force, weighting potentials psi_g, each behind a source voltage
 * V_g(t), a series resistance R_g >= 0 and a stray capacitance Cp_g >= 0 to ground in parallel; the unknown is the
 * conductor's potential U_g.  R_g = 0 is an ideal source: U_g = V_g(t), which still enters the others' equations
 * through C_gh and G_gh.  For time-varying electrode voltages Ramo's theorem gives the current from the lead into
 * electrode g as
 *     I_g = e cond_g + eps0 sum_h C_gh dU_h/dt
 * (cond_g: fedm_currents.conduction[g]; C_gh: fedm_currents.capacitance[g][h]): fedm_currents' total written without
 * the state's time derivative -- the two differ by eps0 sum W grad(D_t Phi_sc) . grad psi_g, which vanishes for a
 * discretely harmonic psi_g.  Kirchhoff at a driven electrode:
 *     (V_g - U_g)/R_g - Cp_g dU_g/dt = I_g.
 * (The signs follow from Q_g = -q psi_g(x); with them a vacuum gap charges as the capacitor eps0 C + Cp through R.)
 * In time: dU/dt = a U^{n+1} + (-(1 + w)^2 U^n + w^2 U^{n-1}) / ((1 + w) dt), a = (1 + 2w)/((1 + w) dt), w = dt/dt_old --
 * the variable-step BDF2 quotient of the species rows and of fedm_currents' D_t Phi, implicit in U^{n+1}; dt_old = 1e30
 * on the first step makes it BDF1, as everywhere.  The conduction is linearised about the accepted state,
 *     cond_g^{n+1} ~ cond_g(u^n) + sum_h G_gh (U_h^{n+1} - U_h^n),
 * with the conductance G_gh = sum_cells sum_s Z_s^2 sum_q W mu_s n_s grad psi_g . grad psi_h, the derivative of the
 * conduction sum with respect to U_h at frozen densities and frozen coefficients.  LFA: mu_s at the cell's |E| as the
 * conduction has it, n_s = exp(u_s) or u_s (linear representation); species with a prescribed drift and species that are
 * not 'drift-diffusion-reaction' add 0.  LMEA: the semi-implicit nodal mobilities and the densities at the quadrature
 * points as the residual of the current step has them, species s >= 1 with sign_s^2, those whose flux has a drift part.
 * G is symmetric and not negative; it decides stability, not consistency (U^{n+1} - U^n -> 0 with dt): the coupling is
 * first order in dt.  The driven electrodes' U^{n+1} solve one dense system of at most 8 x 8,
 *     [diag(1/R_g + a Cp_g) + a eps0 C + e G] U = V_g/R_g - e cond_g + e sum_h G_gh U_h^n - Cp_g hist_g
 *                                                 - eps0 sum_h C_gh hist_h - sum_(h ideal) (a eps0 C_gh + e G_gh) V_h,
 * rows and columns of the driven ones, by Gaussian elimination with partial pivoting on the device.
 * Units: axisymmetric models give amperes, farads, ohms and siemens; in planar models everything is per metre of depth
 * (A/m, F/m, ohm m, S/m).
 * fedm_state_snapshot and fedm_state_restore do NOT cover the circuit's history (U, U_old, U_old1 and the measured
 * quantities): a caller that restores a snapshot sets the circuit up again or keeps its own copy (fedm_circuit_get). */
#define FEDM_VACUUM_PERMITTIVITY 8.854187817e-12   /* fedm/physical_constants.py:7 */
typedef struct {
    int32_t n, pad_;                            /* the n_psi of the currents set-up                                     */
    double R[FEDM_CURRENTS_MAX];                /* series resistance [ohm], 0: ideal source                             */
    double Cp[FEDM_CURRENTS_MAX];               /* stray capacitance to ground [F]                                      */
    double U0[FEDM_CURRENTS_MAX];               /* the conductors' potentials at the start: U = U_old = U_old1          */
    const int8_t *electrode_of_entry;           /* [n_dirichlet] in the order of fedm_mesh_desc.dirichlet_dofs (that of
                                                   fedm_set_dirichlet_values): the electrode whose U the entry gets, -1:
                                                   the entry is left alone                                              */
} fedm_circuit_desc;
#define FEDM_CIRCUIT_NOT_FINITE 1   /* the measured state, cond or G was not finite                                     */
#define FEDM_CIRCUIT_SINGULAR 2     /* the system's pivot was 0 or not finite                                           */
#define FEDM_CIRCUIT_BAD_RESULT 4   /* a U^{n+1} was not finite (a V, dt)                                               */
struct fedm_circuit_state {
    double U[FEDM_CURRENTS_MAX];                /* the last advance's U^{n+1}; before the first, U0                     */
    double U_old[FEDM_CURRENTS_MAX];            /* U^n                                                                  */
    double U_old1[FEDM_CURRENTS_MAX];           /* U^{n-1}                                                              */
    double dUdt[FEDM_CURRENTS_MAX];             /* the BDF2 quotient of the last advance [V/s]                          */
    double lead_current[FEDM_CURRENTS_MAX];     /* of the last advance: (V - U)/R [A]; for an ideal source the linearised
                                                   I_g + Cp_g dU_g/dt                                                   */
    double conduction[FEDM_CURRENTS_MAX];       /* cond_g of the last measure [1/s]                                     */
    double conductance[FEDM_CURRENTS_MAX][FEDM_CURRENTS_MAX];   /* G_gh of the last measure [1/(V s)]                   */
    int32_t n, flag;                            /* flag: 0 or FEDM_CIRCUIT_* of the last advance (before it: of the
                                                   last measure)                                                        */
};
/* Copies the descriptor; U = U_old = U_old1 = U0; the capacitance of the currents set-up goes to the device.  Replaces
 * an earlier set-up.  Refused (-2, fedm_last_error says why): no Poisson equation; a context with ghost vertices or a
 * transport; no currents set-up, or one with another n; an R, Cp or U0 that is negative (R, Cp) or not finite; an entry
 * mapped to an electrode outside 0..n-1 (-1 apart); a null argument, or no map in a context with Dirichlet entries. */
int fedm_circuit_setup(fedm_ctx *ctx, const fedm_circuit_desc *desc);
/* After an accepted step (and once before the first): U_old1 <- U_old <- U, then the currents' cell pass and the
 * conductance pass at u_new (LMEA: with the field table as it stands), finished on the device in a fixed order without
 * floating-point atomics.  No read-back and no synchronisation.  Refused (-2): no circuit set-up; a currents set-up
 * that has since changed its n. */
int fedm_circuit_measure(fedm_ctx *ctx);
/* U^{n+1} for the context's dt and dt_old (fedm_set_step) and the sources' voltages V at the new time, written into
 * the Dirichlet values of the mapped entries; every other entry keeps its value.  A pure function of the last measure,
 * the history, the step and V: a rejected step that is retried with a smaller dt calls it again.  A state that was not
 * finite, a singular system or a result that is not finite set the flag and leave U as it was (the entries then get
 * that U).  out (unless NULL) is read back -- the only synchronisation; U_old, U_old1, conduction and conductance as
 * fedm_circuit_get.  Returns 0 also with a flag.  Refused (-2): no set-up; no fedm_circuit_measure since the set-up; a
 * null V. */
int fedm_circuit_advance(fedm_ctx *ctx, const double V[FEDM_CURRENTS_MAX], struct fedm_circuit_state *out);
/* What the device holds.  Refused (-2): no set-up; a null argument. */
int fedm_circuit_get(fedm_ctx *ctx, struct fedm_circuit_state *out);

/* ---- dielectric-coated electrodes (LFA models, one GPU, coupled step) ---------------------------------------------
 * A boundary tag T may be a dielectric layer of thickness d_T and relative permittivity epsr_T with a conductor at
 * voltage U_T behind it, treated as one-dimensional along the outward normal n (thin layer, no conduction along the
 * solid).  With the surface charge density sigma the potential's natural condition on T is
 *     dPhi/dn = sigma/eps0 - epsr_T (Phi - U_T)/d_T,        d sigma/dt = e sum_s Z_s Gamma_s . n,
 * Gamma_s . n being whatever wall term species s has on T (the 'flux source' expression with its emission, the Neumann
 * drift term, nothing for 'zero flux').  The device keeps, per vertex a of a layer, the charge moment
 *     q_a = int_T sigma phi_a 2 pi r ds    [C; C/m planar]
 * and its history.  W_a,s(u): what the facet kernels add to residual entry (a, s) on the layer's facets.  With
 * w = dt/dt_old the charge is a function of the iterate,
 *     q_a(u) = [(1 + w)^2 q_a^n - w^2 q_a^(n-1)]/(1 + 2w) + dt (1 + w)/(1 + 2w) e sum_s Z_s W_a,s(u),
 * the variable-step BDF2 quotient of the species rows, so plasma charge + surface charge is conserved by the scheme.
 * The Poisson row of a layer vertex gains, in its own measure and scaling (charge_over_eps),
 *     R_Phi,a += sum_q W_q (epsr_T/d_T)(Phi_q - U_T) phi_a - q_a(u)/eps0
 * and the Jacobian its exact derivative: the Robin mass term in the (Phi, Phi) plane, and every entry (a, b, s, col, v)
 * that a layer facet makes in a species row mirrored as (a, b, Phi, col, -kappa Z_s v), kappa = charge_over_eps
 * dt (1 + w)/(1 + 2w).  The (Phi, Phi) plane of such a context is therefore not constant (fedm_plane_masks).
 * fedm_jacobian_poisson_only and fedm_poisson_solve (species frozen) hold the Robin term and the accepted charge
 * q^n alone -- nothing of the mirror, which depends on the iterate: the multigrid hierarchy is built from that plane.
 * A vertex that is on a layer and a Dirichlet vertex of the potential keeps its Dirichlet row; its q_a is kept all the
 * same.  A vertex on facets of several layers counts for the lowest of their tags in the totals. */
typedef struct {
    int32_t is_layer[FEDM_MAX_TAGS];    /* 1: tag t + 1 is a layer                                                     */
    double thickness[FEDM_MAX_TAGS];    /* d [m], > 0                                                                  */
    double eps_r[FEDM_MAX_TAGS];        /* relative permittivity, > 0                                                  */
    double voltage[FEDM_MAX_TAGS];      /* U at the start [V] (fedm_dielectric_set_voltage)                            */
} fedm_dielectric_desc;
struct fedm_dielectric_totals {
    double charge[FEDM_MAX_TAGS];        /* sum_a q_a of the tag's vertices [C; C/m planar]                            */
    double displacement[FEDM_MAX_TAGS];  /* eps0 epsr/d int (Phi - U) 2 pi r ds over the tag's facets, at u_new        */
    double voltage[FEDM_MAX_TAGS];       /* U as it stands                                                             */
    int32_t n_layer_vertices, pad_;
};
/* fedm_ctx_create_walls with layers (walls null: none; layers null or without a layer: that call, kernel for kernel).
 * q = q_old = 0 at the start.  Refused (-2, nothing allocated, fedm_last_error says why and names the tag): a layer on
 * a model without the Poisson equation; a context with ghost vertices (one GPU only); d or epsr that is not finite or
 * not positive; a voltage that is not finite; a layer tag beyond the model's n_tags.  Layer models run the
 * second-generation assembly, never the one-pass kernels, and never the facets' launch fused with the Dirichlet rows
 * when a layer vertex has a Dirichlet row of the potential. */
int fedm_ctx_create_dielectric(const fedm_mesh_desc *mesh, const fedm_model_desc *model, const fedm_wall_desc *walls,
                               const fedm_dielectric_desc *layers, int n_tables, const int32_t *tab_ptr,
                               const double *tab_x, const double *tab_y, int device, fedm_ctx **out);
/* The calls below are refused (-2) on an LMEA context ("the LMEA family has no dielectric layers") and on a context
 * without a layer. */
/* U of every tag (entries of tags that are no layer are ignored), from the next assembly on.  Refused: not finite. */
int fedm_dielectric_set_voltage(fedm_ctx *ctx, const double U[FEDM_MAX_TAGS]);
/* After an accepted step: q_old <- q, q <- q(u_new) with the context's dt and dt_old -- a residual-only pass over the
 * facets, colour by colour without atomics, so two runs give the same bytes.  A rejected step needs nothing undone.
 * No read-back, no synchronisation. */
int fedm_dielectric_accept(fedm_ctx *ctx);
/* The totals (one fixed-order reduction, one read-back) and q, q_old per vertex ([n_vertices], 0 off the layers); any
 * of the three may be null. */
int fedm_dielectric_get(fedm_ctx *ctx, struct fedm_dielectric_totals *totals, double *q, double *q_old);
/* q and q_old per vertex ([n_vertices]; entries off the layers are ignored; null: left alone), for restarts. */
int fedm_dielectric_set(fedm_ctx *ctx, const double *q, const double *q_old);

/* timed micro-benchmarks on the resident state (HIP events on the library's stream):
 * kind 0 = residual+Jacobian assembly, 1 = SpMV, 2 = residual only, 3 = one multigrid cycle on the
 * potential block, 4 = the field split's set-up behind an assembly (species planes), 5 = assembly + that set-up,
 * 6 = species-only residual+Jacobian assembly (fedm_newton_solve_species; the full one where the one-pass kernel does
 * not apply), 7 = the right-hand-side assembly of fedm_poisson_update (residual only).
 * ms per launch. */
int fedm_time_kernel(fedm_ctx *ctx, int kind, int repeats, double *ms_per_launch);
/* Copy rate of the device (GB/s, read + write bytes): a 16-byte-per-lane grid-stride copy between two
 * buffers of `bytes` each -- the practical HBM ceiling bench.py prints next to the specification. */
int fedm_copy_bandwidth(int device, int64_t bytes, int repeats, double *gbs);
/* in-run kernel timing with HIP events on the library's stream.  kind: 0 = assembly F+J,
 * 1 = Jacobian SpMV, 2 = assembly F only, 3 = multigrid V-cycle (whole graph).  Kinds 1 and 3
 * are sampled (every 4th launch carries events; totals are the sampled mean x launches).
 * enable = 1 times the assembly only and leaves the solver untouched; enable = 2 also times
 * kinds 1 and 3, which makes GMRES launch its kernels one by one instead of replaying the
 * captured per-iteration graphs (slower; use it for a separate profiling pass). */
int fedm_profile(fedm_ctx *ctx, int enable);
int fedm_profile_read(fedm_ctx *ctx, int kind, double *ms_total, int64_t *count);
/* assembly kernel: 0 = global graph colouring (bitwise reproducible), 1 = LDS patches
 * (default; each matrix value written once, LDS fp64 atomics) */
int fedm_set_assembly(fedm_ctx *ctx, int kind);
/* side of the field-split preconditioner in the Newton linear solves: 1 = right (flexible GMRES,
 * convergence on the true residual norm; default for LFA models), 0 = left (convergence on the
 * preconditioned residual norm; default for LMEA models; one GPU only: across GPUs the field split
 * is always on the right).  Both solve J delta = -F to ksp_rtol.
 * Environment: FEDM_PRECOND_SIDE=left|right sets the default of new contexts. */
int fedm_set_preconditioner_side(fedm_ctx *ctx, int right);
/* Order of the block-triangular field split when it sits on the right of the operator (the
 * left-preconditioned path is always lower):
 *   0 = lower (default): species sweeps first, then the V-cycle on the potential right-hand side
 *       minus J_phi,u z_u.  The true residual tracks the error of the iterate.
 *   1 = upper: V-cycle on the potential block first, then the species sweeps on t_u - J_u,phi z_phi.
 *       Passes the residual test in 3-4 instead of 8 Krylov steps once a streamer has formed, but
 *       leaves the potential at V-cycle accuracy: the unscaled residual norm (PETSc's and this
 *       library's test) is dominated by the species rows and does not see the Poisson row.  2x
 *       faster late in a run, 4e-3 instead of 6e-6 deviation from a tightly solved run after 220
 *       steps of the bench case (tools/fs_order_accuracy.py): an explicit trade, not the default.
 *       With fedm_set_krylov_scaling "rows" this caveat no longer holds: the equilibrated norm sees the
 *       Poisson rows, and return code 0 means the same accuracy whatever the order.
 * Takes effect with the next Jacobian assembly.  Environment: FEDM_FS_ORDER=lower|upper. */
int fedm_set_fieldsplit_order(fedm_ctx *ctx, int upper);
/* Row-equilibrated residual test of the Newton linear solves (PETSc: KSPSetDiagonalScale).  The systems couple species
 * rows of size ~1e15 with a Poisson row of size ~0.1, so |b - J x|_2 sees the species rows only.
 *   mode 0 = none (default): the test is on |b - J x|_2, as before, bit for bit.
 *   mode 1 = rows: for the DOF i = (vertex v, component r), s_i = sqrt(sum_c J[(v,r),(v,c)]^2) over row r of the
 *       vertex's n_eq x n_eq diagonal block, d_i = 1 / s_i, and d_i = 1 where s_i is zero or not finite (identity
 *       rows -- Dirichlet, outermost ghost layer -- get exactly 1).  Flexible GMRES then minimises and tests
 *       |D (b - J x)|_2 against max(ksp_rtol |D b|_2, ksp_atol); the preconditioner is unchanged.  It runs in the inner
 *       product <x, y> = sum_i d_i^2 x_i y_i (the iterates of GMRES on D J M^-1 D^-1): only the reductions change.
 *       d is not normalised (ksp_atol is compared with |D r|_2 for this d) and is recomputed from the Jacobian at the
 *       start of every scaled solve.  The residual norms a solve reports (fedm_debug_linear_solve's rnorm) are the
 *       scaled ones; the Newton loop's own test stays on the unscaled |F| (fedm_newton_report.fnorm0 / fnorm).
 * Other values are refused.  Defined for the field split on the right (one GPU and several): a solve started with
 * mode 1 under point-block Jacobi or with the field split on the left returns a hard error (< 0), it does not
 * ignore the setting -- there the tested residual M^-1 r is equilibrated already. */
int fedm_set_krylov_scaling(fedm_ctx *ctx, int mode);
/* mode (unless NULL) and, unless NULL, d_out[n_vertices * n_eq] in the caller-side layout of fedm_residual: the d of
 * the Jacobian as it stands, i.e. what a scaled solve started now uses (whatever the mode). */
int fedm_get_krylov_scaling(fedm_ctx *ctx, int *mode, double *d_out);
/* value planes of the Jacobian blocks (bit r * n_eq + c = d(row r)/d(unknown c)) that the assembly
 * keeps between assemblies (constant or structurally zero: not recomputed, not written again) and
 * that the Jacobian SpMV skips (structurally zero: no reaction couples the two species): the bytes
 * the roofline model must not count. */
int fedm_plane_masks(fedm_ctx *ctx, uint32_t *kept_planes, uint32_t *zero_planes);
/* sizes the roofline model needs */
int fedm_sizes(fedm_ctx *ctx, int64_t *n_vertices, int64_t *n_cells, int64_t *n_eq,
               int64_t *nnz_blocks, int64_t *stored_blocks, int64_t *n_colours);

#ifdef __cplusplus
}
#endif
#endif /* FEDM_HIP_H */
