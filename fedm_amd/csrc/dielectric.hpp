// Dielectric layers on boundary tags of an LFA model (include/fedm_hip.h, fedm_ctx_create_dielectric and the
// fedm_dielectric_* calls): what the facet kernels (boundary.hip), the layer kernels and the C ABI (dielectric.hip) and
// the context's set-up and teardown (context.cpp) share.
#pragma once
#include "fedm_internal.hpp"

namespace fedm {

// What a facet kernel of a layer model gets by value besides the model: the tags that are layers and, per species, the
// factor -kappa Z_s of the mirrored entries (kappa = charge_over_eps dt (1 + w)/(1 + 2w), w = dt/dt_old)
struct LayerMirror {
    double kz[FEDM_MAX_SPECIES];
    uint32_t tags;   // bit t: tag t + 1 is a layer
    uint32_t pad_;
};

// ... and the layer kernels: per tag epsr/d (0: no layer) and the conductor's voltage
struct LayerTags {
    double c[FEDM_MAX_TAGS];
    double U[FEDM_MAX_TAGS];
};

struct Dielectric {
    fedm_dielectric_desc desc{};   // as created; desc.voltage: as last set
    uint32_t tags = 0;             // LayerMirror::tags
    int n_lv = 0;                  // layer vertices: the vertices of the layers' facets that lie on them
    int *lv = nullptr;             // [n_lv] their vertex numbers, ascending
    int8_t *lv_tag = nullptr;      // [n_lv] the tag a vertex counts for in the totals (the lowest of its layers), from 0
    int *lv_index = nullptr;       // [nv] vertex -> place in lv, -1: none
    double *q = nullptr, *q_old = nullptr;   // [n_lv] q^n, q^(n-1)
    double *acc = nullptr;         // [n_lv] sum_s Z_s W_a,s of the accept pass
    double *totals = nullptr;      // [2 * FEDM_MAX_TAGS]: charge, displacement
};

LayerMirror layer_mirror(const Ctx &c);
LayerTags layer_tags(const Ctx &c);
// The tags' layer vertices and their buffers, from the mesh as the context was given it (after the boundary facets are
// on the device).  dirichlet_on_layer: some layer vertex has a Dirichlet row of the potential.
int dielectric_setup(Ctx &c, const fedm_dielectric_desc &desc, const fedm_mesh_desc &mesh, bool *dirichlet_on_layer);
void dielectric_release(Ctx &c);
// Behind the volume kernel of an assembly: the Robin term of every layer facet (residual and, with `jacobian`, the
// (Phi, Phi) plane) and the history part of q_a in the Poisson rows of the layer vertices.  mode 1 (Poisson row only,
// species frozen): the accepted charge q^n in place of q(u) -- the mirror depends on the iterate and stays out.
void launch_layer_rows(Ctx &c, bool jacobian, int mode);

}  // namespace fedm
