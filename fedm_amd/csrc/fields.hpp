// Field output (include/fedm_hip.h, fedm_fields_setup / fedm_probe_setup / fedm_fields): what the kernels and the C ABI
// in fields.hip share with the context's teardown.
#pragma once
#include "photo.hpp"

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
    // consistent projection: the P1 mass matrix, one right-hand side and the vectors scalar_pcg borrows
    bool have_mass = false;
    EllMat M;
    double *rhs = nullptr;        // [nvp]
    Photo *cg = nullptr;          // r, z, p, q, partials, red alone: Ctx::photo points here for the duration of a solve
    // probes
    int n_points = 0;
    int *p_vert = nullptr;        // [n_points][3]
    double *p_w = nullptr;        // [n_points][3]
    double *p_out = nullptr;      // [FEDM_FIELDS_MAX_REQ][n_points]
};

}  // namespace fedm
