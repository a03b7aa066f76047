// C ABI of libfedm_hip.so (include/fedm_hip.h): photoionisation in the Helmholtz approximation.  Host logic only: the
// kernels are in photo.hip, the conjugate gradients in scalar_cg.hip.  The one place that assigns Ctx::photo.
#include <cmath>
#include <cstring>

#include "photo.hpp"
#include "postproc.hpp"

namespace fedm {

void photo_release(Ctx &c) {
    Photo *ph = c.photo;
    if (!ph) return;
    for (int m = 0; m < PHOTO_MAX_TERMS; ++m) release_hierarchy(ph->A[m], ph->M[m]);
    ph->cg.release();
    void *ptrs[] = {ph->y, ph->g, ph->cell_g, ph->v_ptr, ph->v_idx, ph->zero};
    for (void *p : ptrs)
        if (p) hipFree(p);
    delete ph;
    c.photo = nullptr;
}

namespace {

// 0, or -2 with the message set: nothing has been allocated
int check_desc(const Ctx &c, const fedm_photo_desc &d) {
    const char *who = "fedm_photo_setup";
    if (c.model_kind != 0) return refuse(who, "the LMEA family has no photoionisation source (LFA models only)");
    if (c.comm || c.n_owned != c.nv)
        return refuse(who, "photoionisation runs on one GPU (this context has a transport or ghost vertices)");
    if (d.n_terms < 1 || d.n_terms > PHOTO_MAX_TERMS)
        return refuse(who, std::to_string(d.n_terms) + " Helmholtz terms, 1 to " + std::to_string(PHOTO_MAX_TERMS) + " are possible");
    for (int m = 0; m < d.n_terms; ++m) {
        if (!(d.kappa[m] > 0.0) || !std::isfinite(d.kappa[m]))
            return refuse(who, "kappa[" + std::to_string(m) + "] must be positive and finite");
        if (!std::isfinite(d.c[m])) return refuse(who, "c[" + std::to_string(m) + "] is not finite");
    }
    if (!std::isfinite(d.efficiency)) return refuse(who, "the efficiency is not finite");
    if (d.n_src < 1 || d.n_src > FEDM_MAX_REACTIONS)
        return refuse(who, std::to_string(d.n_src) + " source reactions, 1 to " + std::to_string(FEDM_MAX_REACTIONS) + " are possible");
    for (int k = 0; k < d.n_src; ++k)
        if (d.src_reaction[k] < 0 || d.src_reaction[k] >= c.model.n_reactions)
            return refuse(who, "source reaction index " + std::to_string(d.src_reaction[k]) + " out of range (the model has " +
                               std::to_string(c.model.n_reactions) + " reactions)");
    if (d.target_species_mask == 0) return refuse(who, "no target species");
    if (d.target_species_mask >> c.ns) return refuse(who, "a target species beyond the model's " + std::to_string(c.ns));
    for (int s = 0; s < c.ns; ++s) {
        if (!((d.target_species_mask >> s) & 1u)) continue;
        if (c.model.ext_nodes[s] != 3 || !c.d_ext[s])
            return refuse(who, "target species " + std::to_string(s) + " has no degree-1 source table (ext_nodes = 3)");
        if (c.expr_n_ops[s] != 0)
            return refuse(who, "target species " + std::to_string(s) + " has an Expression program: one source table cannot hold both");
    }
    if (c.model.n_tags < 32 && (d.zero_tag_mask >> c.model.n_tags))
        return refuse(who, "a zero tag beyond the model's " + std::to_string(c.model.n_tags) + " boundary tags");
    return 0;
}

int setup_impl(Ctx &c, const fedm_photo_desc &d, const fedm_photo_hierarchy *terms) {
    const char *who = "fedm_photo_setup";
    Photo &ph = *c.photo;
    ph.desc = d;
    // the mesh as the context holds it: vertex -> (cell, corner) in ascending order, and the zero vertices
    std::vector<int> cells((size_t)3 * c.nc);
    std::vector<int8_t> tags((size_t)3 * c.nc);
    FEDM_HIP_CHECK(hipMemcpy(cells.data(), c.d_cells, sizeof(int) * cells.size(), hipMemcpyDeviceToHost));
    FEDM_HIP_CHECK(hipMemcpy(tags.data(), c.d_ftags, sizeof(int8_t) * tags.size(), hipMemcpyDeviceToHost));
    std::vector<int> v_ptr, v_idx;
    vertex_cell_lists(c.nv, cells, v_ptr, v_idx);
    std::vector<unsigned char> zero((size_t)c.nvp, 0);
    for (int cell = 0; cell < c.nc; ++cell)
        for (int i = 0; i < 3; ++i) {   // facet i lies opposite vertex i
            const int t = tags[3 * (size_t)cell + i];
            if (t < 1 || t > 32 || !((d.zero_tag_mask >> (t - 1)) & 1u)) continue;
            zero[cells[3 * (size_t)cell + (i + 1) % 3]] = 1;
            zero[cells[3 * (size_t)cell + (i + 2) % 3]] = 1;
        }
    if (device_array(ph.v_ptr, v_ptr.data(), v_ptr.size()) || device_array(ph.v_idx, v_idx.data(), v_idx.size()) ||
        device_array(ph.zero, zero.data(), zero.size()))
        return -1;
    const size_t nvp = (size_t)c.nvp;
    if (device_array<double>(ph.y, nullptr, nvp * d.n_terms) || device_array<double>(ph.g, nullptr, nvp) ||
        device_array<double>(ph.cell_g, nullptr, (size_t)3 * c.nc) || ph.cg.alloc(nvp))
        return -1;
    for (int m = 0; m < d.n_terms; ++m) {
        const std::string term = "term " + std::to_string(m) + ": ";
        if (const int rc = upload_hierarchy(c, who, term, terms[m], ph.A[m], ph.M[m])) return rc;
        // the zero vertices' rows must be unit rows: y stays 0 there through every sweep and product
        const fedm_csr &A0 = terms[m].A[0];
        for (int v = 0; v < c.nv; ++v) {
            if (!zero[v]) continue;
            for (int64_t k = A0.indptr[v]; k < A0.indptr[v + 1]; ++k)
                if (A0.values[k] != (A0.indices[k] == v ? 1.0 : 0.0))
                    return refuse(who, term + "the row of zero vertex " + std::to_string(v) + " is not a unit row");
        }
    }
    FEDM_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

}  // namespace
}  // namespace fedm

using namespace fedm;

extern "C" {

int fedm_photo_setup(fedm_ctx *h, const fedm_photo_desc *desc, const fedm_photo_hierarchy *terms) {
    if (!h || !desc || !terms) {
        set_error("fedm_photo_setup: null argument");
        return -2;
    }
    Ctx &c = h->c;
    if (const int rc = check_desc(c, *desc)) return rc;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    photo_release(c);
    c.photo = new Photo();
    const int rc = setup_impl(c, *desc, terms);
    if (rc != 0) photo_release(c);
    return rc;
}

int fedm_photo_update(fedm_ctx *h, double rtol, int max_it, int iterations[4]) {
    if (!h || !h->c.photo) {
        set_error("fedm_photo_update: fedm_photo_setup has not been called");
        return -2;
    }
    Ctx &c = h->c;
    Photo &ph = *c.photo;
    if (!(rtol > 0.0) || max_it < 0) {
        set_error("fedm_photo_update: rtol must be positive and max_it not negative");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    launch_photo_load_vector(c);
    int rc = 0;
    for (int m = 0; m < PHOTO_MAX_TERMS; ++m) {
        int its = 0;
        if (m < ph.desc.n_terms) {
            const ScalarCgResult cg = scalar_pcg(c, ph.cg, ph.A[m], ph.M[m], ph.g, ph.y + (size_t)m * c.nvp, rtol, max_it);
            its = cg.it;
            ph.stats[PH_CG_ITS0 + m] += its;
            ph.stats[PH_VCYCLES] += cg.vcycles;
            const int status = cg.status(rtol);
            if (status == FEDM_DIVERGED_NAN) {
                // a NaN on the way (or an operator that is not positive definite): the term goes back to 0, so that the
                // tables written below are finite and the next update starts from a clean vector, not from the NaN
                rc = FEDM_DIVERGED_NAN;
                FEDM_HIP_CHECK(hipMemsetAsync(ph.y + (size_t)m * c.nvp, 0, sizeof(double) * c.nvp, c.stream));
            } else if (status == FEDM_DIVERGED_LINEAR) {
                ++ph.stats[PH_EXHAUSTED];
                if (rc == 0) rc = FEDM_DIVERGED_LINEAR;
            }
        }
        if (iterations) iterations[m] = its;
    }
    launch_photo_table_write(c);
    ++ph.stats[PH_UPDATES];
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipGetLastError());
    return rc;
}

int fedm_photo_get(fedm_ctx *h, double *y, double *g) {
    if (!h || !h->c.photo) {
        set_error("fedm_photo_get: fedm_photo_setup has not been called");
        return -2;
    }
    Ctx &c = h->c;
    Photo &ph = *c.photo;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    for (int m = 0; y && m < ph.desc.n_terms; ++m)
        FEDM_HIP_CHECK(hipMemcpy(y + (size_t)m * c.nv, ph.y + (size_t)m * c.nvp, sizeof(double) * c.nv, hipMemcpyDeviceToHost));
    if (g) FEDM_HIP_CHECK(hipMemcpy(g, ph.g, sizeof(double) * c.nv, hipMemcpyDeviceToHost));
    return 0;
}

int fedm_photo_stats(fedm_ctx *h, int64_t out[8], int reset) {
    if (!h || (!out && !reset)) {
        set_error("fedm_photo_stats: null argument");
        return -2;
    }
    if (!h->c.photo) {
        set_error("fedm_photo_stats: fedm_photo_setup has not been called");
        return -2;
    }
    Photo &ph = *h->c.photo;
    if (out)
        for (int i = 0; i < 8; ++i) out[i] = ph.stats[i];
    if (reset)
        for (int i = 0; i < 8; ++i) ph.stats[i] = 0;
    return 0;
}

}  // extern "C"
