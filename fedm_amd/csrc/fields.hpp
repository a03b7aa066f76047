// Field output (include/fedm_hip.h, fedm_fields_setup / fedm_probe_setup / fedm_fields and their LMEA counterparts
// fedm_gd_fields_setup / fedm_gd_probe_setup / fedm_gd_fields): what the kernels and the C ABI in fields.hip share with
// the context's teardown and with gd_fields.hip.
#pragma once
#include <functional>
#include <string>

#include "scalar_cg.hpp"

namespace fedm {

constexpr int FIELDS_THREADS = 256;

struct Fields {
    int *v_ptr = nullptr;         // [nv + 1] vertex -> its (cell, corner) pairs, ascending: the order of every sum
    int *v_idx = nullptr;         // cell * 3 + corner
    double *m = nullptr;          // [nvp] lumped mass m_v = sum |det J| / 6 over the vertex's cells in that order (0: padding)
    double *cell_b = nullptr;     // [FEDM_FIELDS_MAX_REQ][nc][3] the cells' local load vectors of one state's projected requests
    double *out = nullptr;        // [FEDM_FIELDS_MAX_REQ][nvp] the nodal results
    double *first = nullptr;      // [FEDM_FIELDS_MAX_REQ][nvp] X(u_old) while X(u_new) is formed (a blend of two states)
    double *h_out = nullptr;      // pinned [FEDM_FIELDS_MAX_REQ][nvp]: the nodal results on their way to the caller's rows
    int *flag = nullptr;          // [1] not-finite flag of a call
    // consistent projection: the P1 mass matrix, one right-hand side and scalar_pcg's scratch
    bool have_mass = false;
    EllMat M;
    double *rhs = nullptr;        // [nvp]
    ScalarCgWork cg;
    // probes
    int n_points = 0;
    int *p_vert = nullptr;        // [n_points][3]
    double *p_w = nullptr;        // [n_points][3]
    double *p_out = nullptr;      // [FEDM_FIELDS_MAX_REQ][n_points]
};

// ---- what the two families' entry points share (fields.hip) -------------------------------------------
// Ctx::fields serves both: a context is of one family for life, so it can only ever have had its own set-up.
// `who`, `setup_name`, `probe_name`: the entry points a refusal names.
// the mass matrix's checks, then the vertex lists, the lumped mass and every buffer of a call; replaces an earlier set-up
int fields_setup_shared(Ctx &c, const fedm_csr *mass, const char *who);
int fields_probe_setup_shared(Ctx &c, int n_points, const int32_t *vertices, const double *weights, const char *who,
                              const char *setup_name);
// the refusals that do not depend on the requests: before them (the set-up, n_req, the blend, projection, rtol) ...
int fields_check_opts(const Ctx &c, const fedm_field_opts &o, int n_req, const char *who, const char *setup_name);
// ... and after them (the consistent projection's needs, probes without points)
int fields_check_projection(const Ctx &c, const fedm_field_opts &o, bool probes, const char *who, const char *setup_name,
                            const char *probe_name);
// launch(u, raw_sums, dst): the family's cell and vertex pass of the state u into dst[n_req][nvp], the projected
// requests as raw load vectors when raw_sums
using FieldsLaunch = std::function<void(const double *u, int raw_sums, double *dst)>;
// One call: the state(s) the blend needs through `launch`, the consistent solves of the requests with slot[k] >= 0, the
// blend, the probes, the pinned read-back and the flag.  Returns 0 or FEDM_DIVERGED_LINEAR.
int fields_run(Ctx &c, const fedm_field_opts &o, int n_req, const int *slot, bool any_projected, const FieldsLaunch &launch,
               double *nodal, double *probes, int32_t *finite, int32_t *cg_iterations);

}  // namespace fedm
