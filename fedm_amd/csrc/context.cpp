// C ABI of libfedm_hip.so (include/fedm_hip.h): the context, its state and its settings.
// Host logic only; every flop of the hot path runs in the .hip files.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "dielectric.hpp"
#include "photo.hpp"
#include "solver.hpp"

namespace fedm {

static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }

void prof_collect(Ctx &c) {
    Prof &p = c.prof;
    if (p.used == 0) return;
    hipStreamSynchronize(c.stream);
    for (int i = 0; i + 1 < p.used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]) == hipSuccess) {
            p.ms[p.kind[i / 2]] += ms;
            p.cnt[p.kind[i / 2]]++;
        }
    }
    p.used = 0;
}

void prof_begin(Ctx &c, int kind) {
    Prof &p = c.prof;
    p.recording = false;
    if (!p.on || c.capturing || ((kind == 1 || kind == 3) && !p.all_kinds)) return;
    // events cost a few microseconds of stream time each: short, frequent kernels are sampled
    p.recording = (p.seen[kind]++ % p.stride[kind]) == 0;
    if (!p.recording) return;
    if (p.used + 2 > (int)p.ev.size()) prof_collect(c);
    p.kind[p.used / 2] = kind;
    hipEventRecord(p.ev[p.used], c.stream);
}

void prof_end(Ctx &c) {
    Prof &p = c.prof;
    if (!p.on || !p.recording || c.capturing) return;
    hipEventRecord(p.ev[p.used + 1], c.stream);
    p.used += 2;
    p.recording = false;
}

template <class T>
static int upload(T *&dst, const T *src, size_t n) {
    FEDM_HIP_CHECK(hipMalloc((void **)&dst, sizeof(T) * std::max<size_t>(n, 1)));
    if (n) FEDM_HIP_CHECK(hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return 0;
}

static int alloc_zero(double *&p, size_t n, hipStream_t st) {
    FEDM_HIP_CHECK(hipMalloc((void **)&p, sizeof(double) * std::max<size_t>(n, 1)));
    FEDM_HIP_CHECK(hipMemsetAsync(p, 0, sizeof(double) * std::max<size_t>(n, 1), st));
    return 0;
}

static int check_model(const fedm_model_desc &m) {
    if (m.n_species < 1 || m.n_species > FEDM_MAX_SPECIES) return 1;
    if (m.n_reactions < 0 || m.n_reactions > FEDM_MAX_REACTIONS) return 1;
    if (m.n_qp < 1 || m.n_qp > FEDM_MAX_QP || m.n_fqp < 0 || m.n_fqp > FEDM_MAX_FQP) return 1;
    if (m.n_tags < 0 || m.n_tags > FEDM_MAX_TAGS) return 1;
    const int ns = m.n_species, po = m.poisson ? 1 : 0;
    const bool ok = (ns == 1) || (ns == 2) || ((ns == 3 || ns == 4) && po);
    if (!ok) return 1;
    for (int s = 0; s < ns; ++s) {
        if (m.eq_type[s] < 0 || m.eq_type[s] > 2) return 1;
        if (m.mu[s].n_terms < 0 || m.mu[s].n_terms > FEDM_MAX_TERMS) return 1;
        if (m.D[s].n_terms < 0 || m.D[s].n_terms > FEDM_MAX_TERMS) return 1;
        if (m.ext_nodes[s] < 0 || m.ext_nodes[s] > FEDM_MAX_EXT_NODES) return 1;
    }
    for (int j = 0; j < m.n_reactions; ++j)
        if (m.k[j].n_terms < 0 || m.k[j].n_terms > FEDM_MAX_TERMS) return 1;
    return 0;
}

// the tables of fedm_ctx_create_tabulated as the caller passed them (checked by check_tables before anything is allocated)
struct HostTables {
    int n = 0;
    const int32_t *ptr = nullptr;
    const double *x = nullptr, *y = nullptr;
    const char *who = "fedm_ctx_create";   // the entry point, for the messages
    const fedm_wall_desc *walls = nullptr; // fedm_ctx_create_walls (checked by check_walls)
    const fedm_dielectric_desc *layers = nullptr;   // fedm_ctx_create_dielectric (checked by check_layers); null: no layer
};

// Every table reference of the model against the tables: 0, or 1 with the message set.  The kernels trust both.
static int check_tables(const fedm_model_desc &m, const HostTables &t) {
    const std::string who = std::string(t.who) + ": ";
    if (t.n < 0 || t.n > FEDM_MAX_TABLES) {
        set_error(who + std::to_string(t.n) + " tables, at most " + std::to_string(FEDM_MAX_TABLES));
        return 1;
    }
    if (t.n > 0 && !t.ptr) {
        set_error(who + "null tab_ptr");
        return 1;
    }
    if (t.ptr && t.ptr[0] != 0) {
        set_error(who + "tab_ptr must start at 0");
        return 1;
    }
    for (int k = 0; k < t.n; ++k)
        if (t.ptr[k + 1] < t.ptr[k]) {
            set_error(who + "tab_ptr must not decrease (table " + std::to_string(k) + ")");
            return 1;
        }
    const int total = t.n > 0 ? t.ptr[t.n] : 0;
    if (total > FEDM_MAX_TABLE_KNOTS) {
        set_error(who + std::to_string(total) + " knots in all, at most " + std::to_string(FEDM_MAX_TABLE_KNOTS));
        return 1;
    }
    if (total > 0 && (!t.x || !t.y)) {
        set_error(who + "null table arrays");
        return 1;
    }
    for (int k = 0; k < t.n; ++k) {
        const int b = t.ptr[k], e = t.ptr[k + 1];
        if (e == b) {
            set_error(who + "table " + std::to_string(k) + " has no entries");
            return 1;
        }
        for (int i = b; i < e; ++i) {
            if (!std::isfinite(t.x[i]) || !std::isfinite(t.y[i])) {
                set_error(who + "table " + std::to_string(k) + " has a knot or value that is not finite (entry " +
                          std::to_string(i - b) + ")");
                return 1;
            }
            if (i > b && !(t.x[i] > t.x[i - 1])) {
                set_error(who + "the knots of table " + std::to_string(k) + " do not strictly increase (entry " +
                          std::to_string(i - b) + ")");
                return 1;
            }
        }
    }
    auto refs_ok = [&](const fedm_termsum &ts, const char *name, int idx) {
        if (ts.pad_ == 0) return true;
        const std::string coef = std::string(name) + "[" + std::to_string(idx) + "]";
        if (!m.poisson) {
            set_error(who + coef + " refers to a table, but the model has no Poisson equation (no |E|)");
            return false;
        }
        const int r1 = ts.pad_ & 0xffff, r2 = (ts.pad_ >> 16) & 0xffff;
        for (int r : {r1, r2})
            if (r > t.n) {
                set_error(who + coef + " refers to table " + std::to_string(r - 1) + ", " + std::to_string(t.n) +
                          " tables were passed");
                return false;
            }
        if (r1 == 0) {
            set_error(who + coef + " has a second table factor without a first");
            return false;
        }
        return true;
    };
    for (int s = 0; s < m.n_species; ++s)
        if (!refs_ok(m.mu[s], "mu", s) || !refs_ok(m.D[s], "D", s)) return 1;
    for (int j = 0; j < m.n_reactions; ++j)
        if (!refs_ok(m.k[j], "k", j)) return 1;
    return 0;
}

// a (tag, species) of the model is a 'flux source' wall
static bool has_walls(const fedm_model_desc &m) {
    for (int t = 0; t < m.n_tags; ++t)
        for (int s = 0; s < m.n_species; ++s)
            if (m.bc_kind[t][s] == FEDM_BC_FLUX_SOURCE) return true;
    return false;
}

// the species of a 'flux source' entry that the facet kernels give an emission term (element.hpp, wall_facet)
static bool wall_emitter(const fedm_model_desc &m, const fedm_wall_desc &w, int t, int s) {
    return m.bc_kind[t][s] == FEDM_BC_FLUX_SOURCE && m.eq_type[s] == FEDM_EQ_DRIFT_DIFFUSION_REACTION && w.emits[s] != 0;
}

// Every 'flux source' entry of the model against the wall description: 0, or 1 with the message set (it names the tag
// as the mesh numbers it, from 1, and the species).  The kernels trust both.
static int check_walls(const fedm_model_desc &m, const HostTables &t) {
    const std::string who = std::string(t.who) + ": ";
    if (!has_walls(m)) return 0;
    const fedm_wall_desc *w = t.walls;
    for (int tg = 0; tg < m.n_tags; ++tg) {
        const std::string tag = "tag " + std::to_string(tg + 1);
        bool any = false, emitter = false;
        for (int s = 0; s < m.n_species; ++s) {
            if (m.bc_kind[tg][s] != FEDM_BC_FLUX_SOURCE) continue;
            const std::string at = "'flux source' on " + tag + ", species " + std::to_string(s);
            any = true;
            if (!w) {
                set_error(who + at + " needs a wall description (fedm_ctx_create_walls)");
                return 1;
            }
            if (!m.poisson) {
                set_error(who + at + ": the model has no Poisson equation (no E; the facet kernels need one)");
                return 1;
            }
            if (!std::isfinite(w->ref[tg][s]) || 1.0 + w->ref[tg][s] == 0.0) {
                set_error(who + at + ": the reflection coefficient must be finite and not -1");
                return 1;
            }
            if (!std::isfinite(w->vth[tg][s]) || w->vth[tg][s] < 0.0) {
                set_error(who + at + ": the thermal velocity must be finite and not negative");
                return 1;
            }
            if (m.eq_type[s] == FEDM_EQ_DRIFT_DIFFUSION_REACTION && m.has_drift_w[s]) {
                set_error(who + at + ": a species with a constant drift velocity (has_drift_w) cannot meet a wall");
                return 1;
            }
            emitter = emitter || wall_emitter(m, *w, tg, s);
        }
        if (!any) continue;
        if (!std::isfinite(w->gamma[tg])) {
            set_error(who + "the secondary emission coefficient of " + tag + " is not finite");
            return 1;
        }
        if (w->gamma[tg] != 0.0 && !emitter) {
            set_error(who + "secondary emission on " + tag + " (gamma = " + std::to_string(w->gamma[tg]) +
                      "), but none of its 'flux source' drift-diffusion species has emits");
            return 1;
        }
    }
    return 0;
}

// Every layer of the description against the model and the mesh: 0, or 1 with the message set (it names the tag as the
// mesh numbers it, from 1).
static int check_layers(const fedm_model_desc &m, const fedm_mesh_desc &mesh, const HostTables &t) {
    const std::string who = std::string(t.who) + ": ";
    if (!t.layers) return 0;
    for (int tg = 0; tg < FEDM_MAX_TAGS; ++tg) {
        if (!t.layers->is_layer[tg]) continue;
        const std::string at = "the dielectric layer on tag " + std::to_string(tg + 1);
        if (tg >= m.n_tags) {
            set_error(who + at + ": the model has " + std::to_string(m.n_tags) + " boundary tags");
            return 1;
        }
        if (!m.poisson) {
            set_error(who + at + ": the model has no Poisson equation (the layer is a condition on the potential)");
            return 1;
        }
        if (mesh.n_owned_vertices > 0 && mesh.n_owned_vertices < mesh.n_vertices) {
            set_error(who + at + ": the mesh has ghost vertices; layers run on one GPU only");
            return 1;
        }
        if (!std::isfinite(t.layers->thickness[tg]) || t.layers->thickness[tg] <= 0.0) {
            set_error(who + at + ": the thickness d must be finite and positive");
            return 1;
        }
        if (!std::isfinite(t.layers->eps_r[tg]) || t.layers->eps_r[tg] <= 0.0) {
            set_error(who + at + ": the relative permittivity eps_r must be finite and positive");
            return 1;
        }
        if (!std::isfinite(t.layers->voltage[tg])) {
            set_error(who + at + ": the voltage is not finite");
            return 1;
        }
    }
    return 0;
}

// {fedm_model_desc; ModelTables; x; y; [fedm_wall_desc]} in one device allocation (fedm_internal.hpp, ModelTables)
static int upload_model(fedm_model_desc *&dst, const fedm_model_desc &m, const HostTables &t) {
    const int total = t.n > 0 ? t.ptr[t.n] : 0;
    const size_t wall_at = sizeof(fedm_model_desc) + sizeof(ModelTables) + sizeof(double) * 2 * (size_t)total;
    std::vector<unsigned char> buf(wall_at + (t.walls ? sizeof(fedm_wall_desc) : 0));
    if (t.walls) std::memcpy(buf.data() + wall_at, t.walls, sizeof(fedm_wall_desc));
    std::memcpy(buf.data(), &m, sizeof(m));
    ModelTables mt{};
    mt.n_tables = t.n;
    mt.n_knots = total;
    for (int k = 0; k <= t.n && t.n > 0; ++k) mt.ptr[k] = t.ptr[k];
    std::memcpy(buf.data() + sizeof(m), &mt, sizeof(mt));
    if (total) {
        std::memcpy(buf.data() + sizeof(m) + sizeof(mt), t.x, sizeof(double) * total);
        std::memcpy(buf.data() + sizeof(m) + sizeof(mt) + sizeof(double) * total, t.y, sizeof(double) * total);
    }
    FEDM_HIP_CHECK(hipMalloc((void **)&dst, buf.size()));
    FEDM_HIP_CHECK(hipMemcpy(dst, buf.data(), buf.size(), hipMemcpyHostToDevice));
    return 0;
}

int put_vec(Ctx &c, double *dst, const double *src) {
    if (!src) return 0;
    std::memcpy(c.h_stage, src, sizeof(double) * c.n);
    FEDM_HIP_CHECK(hipMemcpyAsync(dst, c.h_stage, sizeof(double) * c.n, hipMemcpyHostToDevice, c.stream));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    return 0;
}

int get_vec(Ctx &c, double *dst, const double *src) {
    FEDM_HIP_CHECK(hipMemcpyAsync(c.h_stage, src, sizeof(double) * c.n, hipMemcpyDeviceToHost, c.stream));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    std::memcpy(dst, c.h_stage, sizeof(double) * c.n);
    return 0;
}

}  // namespace fedm

using namespace fedm;

extern "C" {

const char *fedm_last_error(void) { return g_error.c_str(); }
int fedm_abi_version(void) { return FEDM_ABI_VERSION; }

static int ctx_create_impl(const fedm_mesh_desc *mesh, const fedm_model_desc *model,
                           const fedm_gd_desc *gd, const HostTables &tables, int device, fedm_ctx **out);

// every error exit of the set-up releases what had been allocated so far (context, stream, device
// and pinned memory): a caller that retries after an out-of-memory must not accumulate leaked HBM
static int ctx_create_guarded(const fedm_mesh_desc *mesh, const fedm_model_desc *model,
                              const fedm_gd_desc *gd, const HostTables &tables, int device, fedm_ctx **out) {
    *out = nullptr;
    fedm_ctx *h = nullptr;
    const int rc = ctx_create_impl(mesh, model, gd, tables, device, &h);
    if (rc != 0) {
        const std::string msg = g_error;  // destroy may overwrite it
        if (h) fedm_ctx_destroy(h);
        g_error = msg;
        return rc;
    }
    *out = h;
    return 0;
}

static int ctx_create_lfa(const fedm_mesh_desc *mesh, const fedm_model_desc *model, const HostTables &tables,
                          int device, fedm_ctx **out) {
    if (!mesh || !model || !out) {
        set_error("null argument");
        return -2;
    }
    if (check_model(*model)) {
        // refused, never truncated: the LFA kernels are instantiated for 1-2 species without and 1-4 species
        // with a Poisson equation (fedm_model_desc's arrays hold FEDM_MAX_SPECIES = 4 and FEDM_MAX_REACTIONS = 8)
        set_error("unsupported LFA model: " + std::to_string(model->n_species) + " species" +
                  (model->poisson ? " + Poisson" : "") + ", " + std::to_string(model->n_reactions) +
                  " reactions, " + std::to_string(model->n_qp) + " quadrature points (supported: 1-2 species, or 1-4 "
                  "with a Poisson equation; at most " + std::to_string(FEDM_MAX_REACTIONS) + " reactions, " +
                  std::to_string(FEDM_MAX_TERMS) + " terms per coefficient, " + std::to_string(FEDM_MAX_QP) +
                  " quadrature points)");
        return -2;
    }
    if (check_tables(*model, tables) || check_walls(*model, tables) || check_layers(*model, *mesh, tables)) return -2;
    return ctx_create_guarded(mesh, model, nullptr, tables, device, out);
}

int fedm_ctx_create(const fedm_mesh_desc *mesh, const fedm_model_desc *model, int device,
                    fedm_ctx **out) {
    return ctx_create_lfa(mesh, model, HostTables{}, device, out);
}

int fedm_ctx_create_tabulated(const fedm_mesh_desc *mesh, const fedm_model_desc *model, int n_tables,
                              const int32_t *tab_ptr, const double *tab_x, const double *tab_y, int device,
                              fedm_ctx **out) {
    HostTables t;
    t.n = n_tables;
    t.ptr = tab_ptr;
    t.x = tab_x;
    t.y = tab_y;
    t.who = "fedm_ctx_create_tabulated";
    if (n_tables > 0 && !tab_ptr) {
        set_error("fedm_ctx_create_tabulated: null tab_ptr");
        return -2;
    }
    if (n_tables == 0) t.ptr = nullptr;   // (no tables: fedm_ctx_create)
    return ctx_create_lfa(mesh, model, t, device, out);
}

int fedm_ctx_create_walls(const fedm_mesh_desc *mesh, const fedm_model_desc *model, const fedm_wall_desc *walls,
                          int n_tables, const int32_t *tab_ptr, const double *tab_x, const double *tab_y, int device,
                          fedm_ctx **out) {
    HostTables t;
    t.n = n_tables;
    t.ptr = tab_ptr;
    t.x = tab_x;
    t.y = tab_y;
    t.who = "fedm_ctx_create_walls";
    t.walls = walls;
    if (n_tables > 0 && !tab_ptr) {
        set_error("fedm_ctx_create_walls: null tab_ptr");
        return -2;
    }
    if (n_tables == 0) t.ptr = nullptr;
    return ctx_create_lfa(mesh, model, t, device, out);
}

int fedm_ctx_create_dielectric(const fedm_mesh_desc *mesh, const fedm_model_desc *model, const fedm_wall_desc *walls,
                               const fedm_dielectric_desc *layers, int n_tables, const int32_t *tab_ptr,
                               const double *tab_x, const double *tab_y, int device, fedm_ctx **out) {
    HostTables t;
    t.n = n_tables;
    t.ptr = tab_ptr;
    t.x = tab_x;
    t.y = tab_y;
    t.who = "fedm_ctx_create_dielectric";
    t.walls = walls;
    // (a description without a layer: fedm_ctx_create_walls, kernel for kernel)
    for (int tg = 0; layers && tg < FEDM_MAX_TAGS; ++tg)
        if (layers->is_layer[tg]) t.layers = layers;
    if (n_tables > 0 && !tab_ptr) {
        set_error("fedm_ctx_create_dielectric: null tab_ptr");
        return -2;
    }
    if (n_tables == 0) t.ptr = nullptr;
    return ctx_create_lfa(mesh, model, t, device, out);
}

int fedm_ctx_create_gd(const fedm_mesh_desc *mesh, const fedm_gd_desc *gd, int device,
                       fedm_ctx **out) {
    if (!mesh || !gd || !out) {
        set_error("null argument");
        return -2;
    }
    if (gd->n_species < 2 || gd->n_species > FEDM_GD_MAX_SPECIES - 1 || gd->n_reactions < 0 ||
        gd->n_reactions > FEDM_GD_MAX_REACTIONS || gd->n_qp < 1 || gd->n_qp > FEDM_MAX_QP ||
        gd->n_fqp < 0 || gd->n_fqp > FEDM_MAX_FQP || gd->n_tags < 0 || gd->n_tags > FEDM_MAX_TAGS) {
        set_error("unsupported LMEA model descriptor");
        return -2;
    }
    for (int j = 0; j < gd->n_reactions; ++j)
        for (int i = 0; i < gd->n_species; ++i)
            if (gd->power[j][i] < 0 || gd->power[j][i] > 15) {   // the kernels pack them 4 bits each
                set_error("LMEA reaction powers must be between 0 and 15");
                return -2;
            }
    return ctx_create_guarded(mesh, nullptr, gd, HostTables{}, device, out);
}

int fedm_gd_prep_setup(fedm_ctx *h, const fedm_csr *mass, int n_tables, const int32_t *tab_ptr,
                       const double *tab_x, const double *tab_y, const fedm_gd_field_prog *progs) {
    Ctx &c = h->c;
    if (c.model_kind != 1 || !mass || !tab_ptr || !progs || n_tables < 0 || mass->n_rows != c.nv) {
        set_error("bad LMEA field-refresh description");
        return -2;
    }
    // what np.interp refuses is refused here, before anything is allocated or launched: the kernel trusts the tables
    if (tab_ptr[0] != 0) {
        set_error("fedm_gd_prep_setup: tab_ptr must start at 0");
        return -2;
    }
    for (int t = 0; t < n_tables; ++t)
        if (tab_ptr[t + 1] < tab_ptr[t]) {
            set_error("fedm_gd_prep_setup: tab_ptr must not decrease");
            return -2;
        }
    if (tab_ptr[n_tables] > 0 && (!tab_x || !tab_y)) {
        set_error("fedm_gd_prep_setup: null table arrays");
        return -2;
    }
    for (int r = 0; r < c.gd_n_fields; ++r) {
        const fedm_gd_field_prog &p = progs[r];
        if (p.kind < FEDM_GDP_KEEP || p.kind > FEDM_GDP_UE_OLD ||
            (p.kind == FEDM_GDP_TABLE && p.arg != FEDM_GDP_ARG_ENERGY && p.arg != FEDM_GDP_ARG_REDFIELD)) {
            set_error("fedm_gd_prep_setup: field program with an unknown kind or argument");
            return -2;
        }
        if ((p.kind == FEDM_GDP_TABLE && (p.table < 0 || p.table >= n_tables)) ||
            (p.kind == FEDM_GDP_SCALED_ROW && (p.src_row < 0 || p.src_row >= c.gd_n_fields))) {
            set_error("fedm_gd_prep_setup: field program refers to a missing table or row");
            return -2;
        }
        if (p.kind == FEDM_GDP_TABLE && tab_ptr[p.table + 1] == tab_ptr[p.table]) {
            set_error("fedm_gd_prep_setup: a field program looks up a table without entries");
            return -2;
        }
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    return gd_prep_setup(c, mass, n_tables, tab_ptr, tab_x, tab_y, progs);
}

int fedm_gd_prep_step(fedm_ctx *h) {
    Ctx &c = h->c;
    if (c.model_kind != 1 || !c.gd_prep) {
        set_error("fedm_gd_prep_setup has not been called");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    const int rc = gd_prep_step(c);
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    return rc;
}

int fedm_gd_update_mean_energy(fedm_ctx *h) {
    Ctx &c = h->c;
    if (c.model_kind != 1) {
        set_error("not an LMEA context");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    gd_update_mean_energy(c);
    return 0;
}

int fedm_gd_get_fields(fedm_ctx *h, double *out) {
    Ctx &c = h->c;
    if (c.model_kind != 1 || !out) {
        set_error("not an LMEA context");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    FEDM_HIP_CHECK(hipMemcpy(out, c.d_gd_fields, sizeof(double) * (size_t)c.gd_n_fields * c.nv, hipMemcpyDeviceToHost));
    return 0;
}

int fedm_gd_set_fields(fedm_ctx *h, const double *fields) {
    Ctx &c = h->c;
    if (c.model_kind != 1 || !fields) {
        set_error("not an LMEA context");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipMemcpyAsync(c.d_gd_fields, fields, sizeof(double) * (size_t)c.gd_n_fields * c.nv,
                                  hipMemcpyHostToDevice, c.stream));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    return 0;
}

static int ctx_create_impl(const fedm_mesh_desc *mesh, const fedm_model_desc *model,
                           const fedm_gd_desc *gd, const HostTables &tables, int device, fedm_ctx **out) {
    if (mesh->n_vertices < 3 || mesh->n_cells < 1) {
        set_error("empty mesh");
        return -2;
    }
    for (int i = 0; i < 3 * mesh->n_cells; ++i)
        if (mesh->cells[i] < 0 || mesh->cells[i] >= mesh->n_vertices) {
            set_error("cell vertex index out of range");
            return -2;
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: libfedm_hip has no CPU fallback");
        return -3;
    }
    FEDM_HIP_CHECK(hipSetDevice(device));
    fedm_ctx *h = new fedm_ctx();
    *out = h;  // from here on the caller (ctx_create_guarded) owns it, error exits included
    Ctx &c = h->c;
    c.device = device;
    const int n_tags_model = model ? model->n_tags : gd->n_tags;
    if (model) {
        c.model = *model;
        for (int s_ = 0; s_ < model->n_species; ++s_)
            c.model_tables = c.model_tables || model->mu[s_].pad_ != 0 || model->D[s_].pad_ != 0;
        for (int j = 0; j < model->n_reactions; ++j) c.model_tables = c.model_tables || model->k[j].pad_ != 0;
        c.model_walls = has_walls(*model);
        c.ns = model->n_species;
        c.poisson = model->poisson != 0;
    } else {  // LMEA: energy + (n_species - 1) particle equations + potential
        c.model_kind = 1;
        c.gd = *gd;
        c.ns = gd->n_species;
        c.poisson = true;
        c.assembly_kind = 0;
    }
    c.neq = c.ns + (c.poisson ? 1 : 0);
    c.nv = mesh->n_vertices;
    c.nc = mesh->n_cells;
    {
        // (Expression sources are tables indexed by (cell, local node): their cells keep their vertex order)
        bool tables = false;
        if (model)
            for (int s_ = 0; s_ < model->n_species; ++s_) tables = tables || model->ext_nodes[s_] > 0;
        build_pattern(*mesh, c.pat, !tables);
    }
    c.nvp = c.pat.nvp;
    c.n_owned = (mesh->n_owned_vertices > 0 && mesh->n_owned_vertices <= c.nv) ? mesh->n_owned_vertices : c.nv;
    c.n_dot = (int64_t)c.n_owned * c.neq;
    c.halo_depth = 1;
    if (mesh->halo_depth > 1 && (mesh->identity_vertices || mesh->n_identity_vertices == 0)) {
        for (int i = 0; i < mesh->n_identity_vertices; ++i)
            if (mesh->identity_vertices[i] < c.n_owned || mesh->identity_vertices[i] >= c.nv) {
                set_error("identity_vertices must be ghost vertices");
                return -2;
            }
        c.halo_depth = mesh->halo_depth;
        c.n_identity = mesh->n_identity_vertices;
        if (upload(c.d_identity, mesh->identity_vertices, (size_t)c.n_identity)) return -1;
    }
    c.n = (int64_t)c.nv * c.neq;
    c.np = (int64_t)c.nvp * c.neq;
    for (int i = 0; i < mesh->n_dirichlet; ++i)
        if (mesh->dirichlet_dofs[i] < 0 || mesh->dirichlet_dofs[i] >= c.n) {
            set_error("Dirichlet dof out of range");
            return -2;
        }
    FEDM_HIP_CHECK(hipStreamCreate(&c.stream));
    if (upload(c.d_coords, mesh->coords, (size_t)2 * c.nv)) return -1;
    if (upload(c.d_cells, mesh->cells, (size_t)3 * c.nc)) return -1;
    std::vector<int8_t> zero_tags;
    const int8_t *tags = mesh->facet_tags;
    if (!tags) {
        zero_tags.assign((size_t)3 * c.nc, 0);
        tags = zero_tags.data();
    }
    for (size_t i = 0; i < (size_t)3 * c.nc; ++i)
        if (tags[i] < 0 || tags[i] > n_tags_model) {
            set_error("facet tag out of range");
            return -2;
        }
    if (upload(c.d_ftags, tags, (size_t)3 * c.nc)) return -1;
    {
        // tagged boundary facets, greedily coloured so that facets of one colour share no
        // vertex of their cells: the boundary kernel can then add without atomics, in a
        // fixed order (bitwise reproducible)
        std::vector<int> fcell, floc, ftag, fcol;
        std::vector<uint32_t> used(c.nv, 0);
        int ncol = 0;
        for (int cell = 0; cell < c.nc; ++cell)
            for (int i = 0; i < 3; ++i)
                if (tags[3 * cell + i] > 0) {
                    const int32_t *v = mesh->cells + 3 * cell;
                    const uint32_t m = used[v[0]] | used[v[1]] | used[v[2]];
                    int k = 0;
                    while (k < 31 && ((m >> k) & 1u)) ++k;
                    for (int a = 0; a < 3; ++a) used[v[a]] |= (1u << k);
                    ncol = std::max(ncol, k + 1);
                    fcell.push_back(cell);
                    floc.push_back(i);
                    ftag.push_back(tags[3 * cell + i]);
                    fcol.push_back(k);
                }
        std::vector<int> bf;
        c.bfacet_colour_ptr.assign(ncol + 1, 0);
        for (int k = 0; k < ncol; ++k) {
            for (size_t f = 0; f < fcell.size(); ++f)
                if (fcol[f] == k) {
                    bf.push_back(fcell[f]);
                    bf.push_back(floc[f]);
                    bf.push_back(ftag[f]);
                }
            c.bfacet_colour_ptr[k + 1] = (int)bf.size() / 3;
        }
        c.n_bfacets = (int)bf.size() / 3;
        if (upload(c.d_bfacets, bf.data(), bf.size())) return -1;
        // Do the boundary facets (species rows of their cells' vertices) and the Dirichlet dofs meet in a row?  If not
        // -- the scripts put Dirichlet values on the potential only -- the two can share a launch (launch_finalize)
        std::vector<char> is_dirichlet((size_t)c.nv * c.neq, 0);
        for (int k = 0; k < mesh->n_dirichlet; ++k)
            if (mesh->dirichlet_dofs[k] >= 0 && (int64_t)mesh->dirichlet_dofs[k] < (int64_t)c.nv * c.neq)
                is_dirichlet[mesh->dirichlet_dofs[k]] = 1;
        c.boundary_rows_disjoint = true;
        for (size_t f = 0; f < fcell.size() && c.boundary_rows_disjoint; ++f)
            for (int a = 0; a < 3; ++a)
                for (int sp = 0; sp < c.ns; ++sp)
                    if (is_dirichlet[(size_t)mesh->cells[3 * fcell[f] + a] * c.neq + sp]) c.boundary_rows_disjoint = false;
        if (tables.layers) {
            // a layer's facets add to the Poisson rows of its vertices as well: a Dirichlet row of the potential
            // among them belongs to both the facets and the Dirichlet rows, so the two keep their own launches
            bool dirichlet_on_layer = false;
            if (const int rc = dielectric_setup(c, *tables.layers, *mesh, &dirichlet_on_layer)) return rc;
            if (dirichlet_on_layer) c.boundary_rows_disjoint = false;
        }
        // the rows that change behind the volume assembly (Ctx::planes_fused): vertices of boundary-facet cells, of
        // Dirichlet values, and the padding of the last slice
        {
            std::vector<char> touched((size_t)c.nvp, 0);
            for (size_t f = 0; f < fcell.size(); ++f)
                for (int a = 0; a < 3; ++a) touched[mesh->cells[3 * fcell[f] + a]] = 1;
            for (int k = 0; k < mesh->n_dirichlet; ++k)
                if (mesh->dirichlet_dofs[k] >= 0 && (int64_t)mesh->dirichlet_dofs[k] < (int64_t)c.nv * c.neq)
                    touched[mesh->dirichlet_dofs[k] / c.neq] = 1;
            for (int v = c.nv; v < c.nvp; ++v) touched[v] = 1;
            std::vector<int> rows;
            for (int v = 0; v < c.nvp; ++v)
                if (touched[v]) rows.push_back(v);
            c.n_planes_rows = (int)rows.size();
            if (c.n_planes_rows && upload(c.d_planes_rows, rows.data(), rows.size())) return -1;
            const char *e = getenv("FEDM_PLANES_FUSED");
            // one GPU, whole-mesh launches: no identity rows of ghost layers, no listed part launches
            // (opt-in, FEDM_PLANES_FUSED=1: measured -9 us per assembly back to back, nothing in the bench's step, and the
            // dominant kernel 75 -> 89 us: DESIGN.md Appendix A)
            c.planes_fuse_ok = (e && e[0] == '1') && mesh->n_identity_vertices == 0 && c.n_owned == c.nv;
        }
    }
    if (upload(c.d_cell_slots, c.pat.cell_slots.data(), c.pat.cell_slots.size())) return -1;
    if (upload(c.d_colour_cells, c.pat.colour_cells.data(), c.pat.colour_cells.size())) return -1;
    if (model) {
        if (upload_model(c.d_model, *model, tables)) return -1;
    } else {
        if (upload(c.d_gd, gd, 1)) return -1;
        c.gd_n_fields = FEDM_GD_N_FIELDS(gd->n_species, gd->n_reactions);
        if (alloc_zero(c.d_gd_fields, (size_t)c.gd_n_fields * c.nv, c.stream)) return -1;
    }
    if (upload(c.d_patch_cell_ptr, c.pat.patch_cell_ptr.data(), c.pat.patch_cell_ptr.size())) return -1;
    if (upload(c.d_patch_halo_ptr, c.pat.patch_halo_ptr.data(), c.pat.patch_halo_ptr.size())) return -1;
    if (upload(c.d_patch_halo, c.pat.patch_halo.data(), c.pat.patch_halo.size())) return -1;
    if (upload(c.d_patch_cells, c.pat.patch_cells.data(), c.pat.patch_cells.size())) return -1;
    {
        // LDS patches need 8-bit local indices and <= 160 KiB of LDS per workgroup; the
        // globally coloured kernel is the (deterministic, slower) alternative.
        const char *env = getenv("FEDM_ASSEMBLY");
        c.assembly_kind = (env && std::string(env) == "colour") ? 0 : 1;
        // Side of the field split: right for the LFA systems (3 instead of 5.25 Krylov steps per
        // Newton iteration on the streamer case); left for LMEA, whose rows (energy balance next to
        // densities) are scaled so differently that the true residual norm is the harder target
        // (glow discharge, 402k DOFs: 70 against 100 steps per time step).  FEDM_PRECOND_SIDE or
        // fedm_set_preconditioner_side override.
        c.right_precond = c.model_kind == 0;
        if (const char *lean = getenv("FEDM_ASSEMBLY_LEAN")) c.assembly_lean = lean[0] == '0' ? 0 : (lean[0] == '3' ? 3 : 2);
        if (const char *e = getenv("FEDM_XCD_REMAP")) c.xcd_remap = e[0] != '0';
        if (const char *e = getenv("FEDM_ASSEMBLY_OVERLAP")) c.assembly_overlap = e[0] != '0';
        if (const char *e = getenv("FEDM_SKIP_CONST_PLANES")) c.skip_const_planes = e[0] != '0';
        if (model && c.poisson) {
            // potential-potential: geometry only.  Species (s, i), i != s: zero unless a reaction that
            // changes species s has species i among its reactants (fedm/functions.py:835-843).
            c.const_plane_mask = 1u << (c.ns * c.neq + c.ns);
            for (int s_ = 0; s_ < c.ns; ++s_)
                for (int i = 0; i < c.ns; ++i) {
                    if (i == s_) continue;
                    bool coupled = false;
                    for (int j = 0; j < model->n_reactions; ++j)
                        coupled = coupled || (model->net[j][s_] != 0 && model->power[j][i] > 0);
                    // ... or a wall gives species s the secondary electrons of ion i (element.hpp, wall_facet): the
                    // facet kernels add to that plane after every volume assembly, so it is neither kept nor skipped
                    for (int tg = 0; tables.walls && tg < model->n_tags; ++tg)
                        coupled = coupled || (wall_emitter(*model, *tables.walls, tg, s_) && tables.walls->gamma[tg] != 0.0 &&
                                              tables.walls->is_ion[i] != 0 && model->eq_type[i] != FEDM_EQ_REACTION);
                    if (!coupled) c.const_plane_mask |= 1u << (s_ * c.neq + i);
                }
            c.zero_plane_mask = c.const_plane_mask & ~(1u << (c.ns * c.neq + c.ns));
            // a layer's facets add the mirrored potential column and the Robin term to the potential-potential plane
            // after every volume assembly: it is written afresh each time, like an emission plane
            if (tables.layers) c.const_plane_mask &= ~(1u << (c.ns * c.neq + c.ns));
            if (const char *e = getenv("FEDM_SPMV_SKIP_ZERO_PLANES"))
                if (e[0] == '0') c.zero_plane_mask = 0;
        }
        if (const char *e = getenv("FEDM_FS_HALO")) c.fs_halo = e[0] != '0';
        if (const char *e = getenv("FEDM_DEEP_HALO")) c.deep_halo = e[0] != '0';
        if (const char *e = getenv("FEDM_FS_POLICY")) c.fs_measured_policy = std::string(e) != "counts";
        if (const char *e = getenv("FEDM_FS_LAGGED_COUPLING")) c.fs_lagged_coupling = e[0] != '0';
        if (const char *e = getenv("FEDM_GD_HAND"))
            if (e[0] == '0' || (e[0] >= '2' && e[0] <= '5')) c.gd_hand_mode = e[0] - '0';
        if (const char *e = getenv("FEDM_GD_WAVES")) c.gd_waves = e[0];
        if (const char *e = getenv("FEDM_GD_GATHER")) c.gd_gather = e[0];
        if (const char *e = getenv("FEDM_FS_ORDER")) c.fs_upper = std::string(e) == "upper";
        const char *side = getenv("FEDM_PRECOND_SIDE");
        if (side && std::string(side) == "left") c.right_precond = false;
        if (side && std::string(side) == "right") c.right_precond = true;
        if (!patch_assembly_available(c)) c.assembly_kind = 0;
    }
    if (upload(c.d_slice_boff, c.pat.slice_boff.data(), c.pat.slice_boff.size())) return -1;
    if (upload(c.d_colidx, c.pat.colidx.data(), c.pat.colidx.size())) return -1;
    if (upload(c.d_diag_slot, c.pat.diag_slot.data(), c.pat.diag_slot.size())) return -1;
    {
        // A Dirichlet dof of a vertex with identity rows (a caller may list the Dirichlet dofs of every local vertex)
        // goes behind the others: dirichlet_kernel writes rows for the first n_dir_rows entries only, so F = 0 and the
        // unit row of the identity branch have one writer.
        std::vector<char> identity_vertex((size_t)c.nv, 0);
        if (c.d_identity)
            for (int i = 0; i < c.n_identity; ++i) identity_vertex[mesh->identity_vertices[i]] = 1;
        else
            for (int v = c.n_owned; v < c.nv; ++v) identity_vertex[v] = 1;
        c.n_dir = mesh->n_dirichlet;
        c.dir_perm.clear();
        for (int pass = 0; pass < 2; ++pass) {
            for (int k = 0; k < c.n_dir; ++k)
                if ((identity_vertex[mesh->dirichlet_dofs[k] / c.neq] != 0) == (pass == 1)) c.dir_perm.push_back(k);
            if (pass == 0) c.n_dir_rows = (int)c.dir_perm.size();
        }
        std::vector<int> dofs((size_t)c.n_dir);
        std::vector<double> vals((size_t)c.n_dir);
        for (int k = 0; k < c.n_dir; ++k) {
            dofs[k] = mesh->dirichlet_dofs[c.dir_perm[k]];
            vals[k] = mesh->dirichlet_vals[c.dir_perm[k]];
        }
        if (upload(c.d_dir_dofs, dofs.data(), (size_t)c.n_dir)) return -1;
        if (upload(c.d_dir_vals, vals.data(), (size_t)c.n_dir)) return -1;
    }
    const size_t nval = (size_t)c.pat.total_bc * SLICE * c.neq * c.neq;
    if (alloc_zero(c.d_val, nval, c.stream)) return -1;
    if (alloc_zero(c.d_dinv, (size_t)c.nvp * c.neq * c.neq, c.stream)) return -1;
    double **vecs[] = {&c.d_u, &c.d_uold, &c.d_uold1, &c.d_F, &c.d_delta, &c.d_w, &c.d_rhs, &c.d_tmp, &c.d_fs, &c.d_fs_g};
    for (auto v : vecs)
        if (alloc_zero(*v, (size_t)c.np, c.stream)) return -1;
    if (alloc_zero(c.d_partials, (size_t)RED_BLOCKS * RED_K, c.stream)) return -1;
    if (alloc_zero(c.d_red, 2 * RED_K, c.stream)) return -1;
    FEDM_HIP_CHECK(hipHostMalloc((void **)&c.h_mail, sizeof(double) * MAIL_SLOTS * (RED_K + 1), hipHostMallocDefault));
    std::memset(c.h_mail, 0, sizeof(double) * MAIL_SLOTS * (RED_K + 1));
    c.h_red = c.h_mail;
    FEDM_HIP_CHECK(hipMalloc((void **)&c.d_mail_seq, sizeof(unsigned long long)));
    FEDM_HIP_CHECK(hipMemset(c.d_mail_seq, 0, sizeof(unsigned long long)));

    FEDM_HIP_CHECK(hipHostMalloc((void **)&c.h_stage, sizeof(double) * (size_t)c.np));
    for (int s = 0; model && s < c.ns; ++s)
        if (model->ext_nodes[s] > 0)
            if (alloc_zero(c.d_ext[s], (size_t)c.nc * model->ext_nodes[s], c.stream)) return -1;
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    return 0;
}

void fedm_ctx_destroy(fedm_ctx *h) {
    if (!h) return;
    Ctx &c = h->c;
    hipSetDevice(c.device);
    // a failed transport first: its communicator is aborted before anything below waits for the device
    // (comm.hip, Comm::release_communicator); the error stays readable through fedm_last_error
    if (c.comm) {
        comm_poll_async_error(c);
        if (c.comm->failed && c.comm->release_communicator())
            set_error(c.comm->error + " -- communicator aborted at teardown");
    }
    if (c.stream) hipStreamSynchronize(c.stream);
    void *ptrs[] = {c.d_coords, c.d_cells, c.d_ftags, c.d_cell_slots, c.d_colour_cells, c.d_model,
                    c.d_slice_boff, c.d_colidx, c.d_diag_slot, c.d_val, c.d_dinv, c.d_dir_dofs,
                    c.d_dir_vals, c.d_identity, c.d_u, c.d_uold, c.d_uold1, c.d_F, c.d_delta, c.d_w, c.d_rhs,
                    c.d_tmp, c.d_fs, c.d_fs_g, c.d_V, c.d_partials, c.d_partials_wide, c.d_red, c.d_ext[0], c.d_ext[1], c.d_ext[2],
                    c.d_ext[3], c.d_patch_cell_ptr, c.d_patch_halo_ptr, c.d_patch_halo,
                    c.d_patch_cells, c.d_bfacets, c.d_gd, c.d_gd_fields, c.d_gd_elem, c.d_gd_inv_ptr,
                    c.d_gd_inv_idx, c.d_gd_elemF, c.d_gd_vinv_ptr, c.d_gd_vinv_idx, c.d_gd_kpos};
    for (void *p : ptrs)
        if (p) hipFree(p);
    for (Amg *a : {c.amg, c.amg_alt})
        if (a) {
            a->release();
            delete a;
        }
    if (c.comm) {
        c.comm->release();
        delete c.comm;
    }
    gd_prep_release(c);
    photo_release(c);
    diag_release(c);
    fields_release(c);
    gd_balance_release(c);
    circuit_release(c);
    dielectric_release(c);
    currents_release(c);
    fs_tiles_release(c);
    for (auto &e : c.prof.ev) hipEventDestroy(e);
    iter_graphs_clear(c);
    if (c.d_mail_seq) hipFree(c.d_mail_seq);
    if (c.h_mail) hipHostFree(c.h_mail);
    if (c.d_val32) hipFree(c.d_val32);
    if (c.d_s16) hipFree(c.d_s16);
    if (c.d_planes_rows) hipFree(c.d_planes_rows);
    if (c.d_Z) hipFree(c.d_Z);
    if (c.d_kscale2) hipFree(c.d_kscale2);
    if (c.h_stage) hipHostFree(c.h_stage);
    if (c.d_snapshot) hipFree(c.d_snapshot);
    if (c.d_seg_dinv) hipFree(c.d_seg_dinv);
    lean3_release(c);
    for (int s_ = 0; s_ < FEDM_MAX_SPECIES; ++s_) {
        if (c.d_expr_ops[s_]) hipFree(c.d_expr_ops[s_]);
        if (c.d_expr_consts[s_]) hipFree(c.d_expr_consts[s_]);
    }
    if (c.stream) hipStreamDestroy(c.stream);
    delete h;
}

int fedm_set_state(fedm_ctx *h, const double *u_new, const double *u_old, const double *u_old1) {
    Ctx &c = h->c;
    c.err_cache_comp = -1;   // the state changes: the kept error norm is stale
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (u_new) c.halo_pending = false;  // the caller's vector carries its own ghost values
    if (put_vec(c, c.d_u, u_new) || put_vec(c, c.d_uold, u_old) || put_vec(c, c.d_uold1, u_old1)) return -1;
    return 0;
}

int fedm_get_state(fedm_ctx *h, double *u_new) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    return get_vec(c, u_new, c.d_u);
}

int fedm_get_state_old(fedm_ctx *h, double *u_old) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    return get_vec(c, u_old, c.d_uold);
}

int fedm_shift_state(fedm_ctx *h) {
    Ctx &c = h->c;
    c.err_cache_comp = -1;   // the state changes: the kept error norm is stale
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    std::swap(c.d_uold1, c.d_uold);  // old1 <- old (by rotation), then old <- new
    launch_scale_copy(c, 1.0, c.d_u, c.d_uold);
    return 0;
}

int fedm_reset_state(fedm_ctx *h) {
    Ctx &c = h->c;
    c.err_cache_comp = -1;   // the state changes: the kept error norm is stale
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    launch_scale_copy(c, 1.0, c.d_uold, c.d_u);
    return 0;
}

int fedm_state_snapshot(fedm_ctx *h) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (c.halo_pending) {   // (several GPUs: the ghost entries of the state are exchanged lazily)
        comm_halo(c, c.d_u);
        c.halo_pending = false;
    }
    if (!c.d_snapshot) FEDM_HIP_CHECK(hipMalloc((void **)&c.d_snapshot, sizeof(double) * 3 * c.np));
    const double *src[3] = {c.d_u, c.d_uold, c.d_uold1};
    for (int k = 0; k < 3; ++k)
        FEDM_HIP_CHECK(hipMemcpyAsync(c.d_snapshot + (size_t)k * c.np, src[k], sizeof(double) * c.np,
                                      hipMemcpyDeviceToDevice, c.stream));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    // ... and what the solver has learnt from the steps before (how many Krylov steps to queue ahead, at which Newton
    // iteration the final check is expected): steps repeated from the checkpoint then run as they did the first time
    c.snap_krylov_steps_hint = c.krylov_steps_hint;
    std::copy(std::begin(c.krylov_hints), std::end(c.krylov_hints), std::begin(c.snap_krylov_hints));
    c.snap_newton_its_hint = c.newton_its_hint;
    return 0;
}

int fedm_state_restore(fedm_ctx *h) {
    Ctx &c = h->c;
    if (!c.d_snapshot) {
        set_error("fedm_state_restore: no snapshot taken");
        return -2;
    }
    c.err_cache_comp = -1;
    c.krylov_steps_hint = c.snap_krylov_steps_hint;
    std::copy(std::begin(c.snap_krylov_hints), std::end(c.snap_krylov_hints), std::begin(c.krylov_hints));
    c.newton_its_hint = c.snap_newton_its_hint;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    c.halo_pending = false;   // the snapshot was taken with exchanged ghosts
    double *dst[3] = {c.d_u, c.d_uold, c.d_uold1};
    for (int k = 0; k < 3; ++k)
        FEDM_HIP_CHECK(hipMemcpyAsync(dst[k], c.d_snapshot + (size_t)k * c.np, sizeof(double) * c.np,
                                      hipMemcpyDeviceToDevice, c.stream));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    return 0;
}

int fedm_set_step(fedm_ctx *h, double dt, double dt_old) {
    h->c.dt = dt;
    h->c.dt_old = dt_old;
    return 0;
}

int fedm_set_dirichlet_values(fedm_ctx *h, const double *vals) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    if (c.n_dir) {
        std::vector<double> ordered((size_t)c.n_dir);   // the context's order (Ctx::dir_perm)
        for (int k = 0; k < c.n_dir; ++k) ordered[k] = vals[c.dir_perm[k]];
        FEDM_HIP_CHECK(hipMemcpy(c.d_dir_vals, ordered.data(), sizeof(double) * c.n_dir, hipMemcpyHostToDevice));
    }
    return 0;
}

int fedm_set_ext_source(fedm_ctx *h, int species, const double *nodal) {
    Ctx &c = h->c;
    if (species < 0 || species >= c.ns || !c.d_ext[species]) {
        set_error("species has no Expression source");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipMemcpyAsync(c.d_ext[species], nodal,
                                  sizeof(double) * (size_t)c.nc * c.model.ext_nodes[species],
                                  hipMemcpyHostToDevice, c.stream));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    return 0;
}

// the program is checked here once (stack discipline, index ranges): the kernel trusts it
int fedm_ext_source_program(fedm_ctx *h, int species, int n_ops, const int32_t *ops, int n_consts,
                            const double *consts, int n_params) {
    Ctx &c = h->c;
    if (species < 0 || species >= c.ns || !c.d_ext[species]) {
        set_error("species has no Expression source");
        return -2;
    }
    if (c.photo && ((c.photo->desc.target_species_mask >> species) & 1u)) {
        set_error("species receives the photoionisation source: one source table cannot hold an Expression program as well");
        return -2;
    }
    const int nodes = c.model.ext_nodes[species];
    if (nodes != 3 && nodes != 6 && nodes != 10) {
        set_error("device evaluation of Expression sources: degree 1, 2 or 3");
        return -2;
    }
    if (!ops || n_ops < 1 || n_ops > FEDM_EXPR_MAX_OPS || n_consts < 0 || (n_consts > 0 && !consts) ||
        n_params < 0 || n_params > FEDM_EXPR_MAX_PARAMS) {
        set_error("bad expression program");
        return -2;
    }
    int depth = 0;
    for (int k = 0; k < n_ops; ++k) {
        const int op = ops[2 * k], arg = ops[2 * k + 1];
        bool ok = true;
        if (op == FEDM_OP_CONST) ok = arg >= 0 && arg < n_consts, ++depth;
        else if (op == FEDM_OP_X) ok = arg == 0 || arg == 1, ++depth;
        else if (op == FEDM_OP_PARAM) ok = arg >= 0 && arg < n_params, ++depth;
        else if (op >= FEDM_OP_ADD && op <= FEDM_OP_POW) ok = depth >= 2, --depth;
        else if (op >= FEDM_OP_NEG && op <= FEDM_OP_ATAN) ok = depth >= 1;
        else ok = false;
        if (!ok || depth > FEDM_EXPR_STACK) {
            set_error("bad expression program (opcode, operand index or stack depth)");
            return -2;
        }
    }
    if (depth != 1) {
        set_error("bad expression program (it must leave one value)");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (c.d_expr_ops[species]) hipFree(c.d_expr_ops[species]);
    if (c.d_expr_consts[species]) hipFree(c.d_expr_consts[species]);
    c.d_expr_ops[species] = nullptr;
    c.d_expr_consts[species] = nullptr;
    c.expr_n_ops[species] = 0;
    FEDM_HIP_CHECK(hipMalloc((void **)&c.d_expr_ops[species], sizeof(int) * 2 * n_ops));
    FEDM_HIP_CHECK(hipMalloc((void **)&c.d_expr_consts[species], sizeof(double) * (n_consts > 0 ? n_consts : 1)));
    FEDM_HIP_CHECK(hipMemcpy(c.d_expr_ops[species], ops, sizeof(int) * 2 * n_ops, hipMemcpyHostToDevice));
    if (n_consts > 0)
        FEDM_HIP_CHECK(hipMemcpy(c.d_expr_consts[species], consts, sizeof(double) * n_consts, hipMemcpyHostToDevice));
    c.expr_n_ops[species] = n_ops;
    c.expr_n_params[species] = n_params;
    return 0;
}

int fedm_ext_source_eval(fedm_ctx *h, int species, const double *params) {
    Ctx &c = h->c;
    if (species < 0 || species >= c.ns || !c.d_ext[species] || c.expr_n_ops[species] == 0) {
        set_error("species has no expression program");
        return -2;
    }
    if (c.expr_n_params[species] > 0 && !params) {
        set_error("null argument");
        return -2;
    }
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    launch_ext_source_eval(c, species, params);
    FEDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int fedm_sync_ghosts(fedm_ctx *h) {
    Ctx &c = h->c;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    comm_halo(c, c.d_u);
    comm_halo(c, c.d_uold);
    comm_halo(c, c.d_uold1);
    c.halo_pending = false;
    FEDM_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (comm_failed(c)) {
        set_error(c.comm->error);
        return -1;
    }
    return 0;
}

int fedm_set_fieldsplit(fedm_ctx *h, int sweeps, const double *weights) {
    if (sweeps < 1 || sweeps > 16 || !weights) {
        set_error("field-split sweeps must be 1..16 with one weight each");
        return -2;
    }
    for (int i = 0; i < sweeps; ++i)
        if (!(weights[i] > 0.0 && weights[i] < 4.0)) {
            set_error("field-split weights must be positive");
            return -2;
        }
    hipSetDevice(h->c.device);
    hipStreamSynchronize(h->c.stream);
    iter_graphs_clear(h->c);
    Ctx &c = h->c;
    set_hard_mode(c, false);
    c.fs_sweeps = c.fs_main_sweeps = sweeps;
    for (int i = 0; i < sweeps; ++i) c.fs_w[i] = c.fs_main_w[i] = weights[i];
    c.fs_alt_sweeps = 0;
    return 0;
}

int fedm_set_fieldsplit_alternative(fedm_ctx *h, int alt_sweeps, const double *alt_weights,
                                    double switch_above, double back_below) {
    Ctx &c = h->c;
    if (alt_sweeps < 0 || alt_sweeps > 16 || (alt_sweeps > 0 && !alt_weights) || !(back_below < switch_above)) {
        set_error("alternative field-split sweeps must be 0..16 with one weight each, back_below < switch_above");
        return -2;
    }
    for (int i = 0; i < alt_sweeps; ++i)
        if (!(alt_weights[i] > 0.0 && alt_weights[i] < 4.0)) {
            set_error("field-split weights must be positive");
            return -2;
        }
    hipSetDevice(c.device);
    set_hard_mode(c, false);  // back to the main set first
    c.fs_alt_sweeps = alt_sweeps;
    for (int i = 0; i < alt_sweeps; ++i) c.fs_alt_w[i] = alt_weights[i];
    c.fs_switch_above = switch_above;
    c.fs_back_below = back_below;
    return 0;
}

int fedm_fieldsplit_policy(fedm_ctx *h, int64_t out[4]) {
    if (!h || !out) return -2;
    const Ctx &c = h->c;
    out[0] = (c.fs_measured_policy && !(c.comm && c.comm->nranks > 1)) ? 1 : 0;
    out[1] = c.fs_alt_active ? 1 : 0;
    out[2] = c.fs_solves[0];
    out[3] = c.fs_solves[1];
    return 0;
}

int fedm_set_assembly(fedm_ctx *h, int kind) {
    Ctx &c = h->c;
    if (kind == 1 && !patch_assembly_available(c)) {
        set_error("LDS patch assembly unavailable for this mesh");
        return -2;
    }
    if (kind != 0 && kind != 1) {
        set_error("assembly kind must be 0 (colouring) or 1 (LDS patches)");
        return -2;
    }
    c.assembly_kind = kind;
    return 0;
}

int fedm_set_preconditioner_side(fedm_ctx *h, int right) {
    Ctx &c = h->c;
    if (right != 0 && right != 1) {
        set_error("preconditioner side must be 0 (left) or 1 (right)");
        return -2;
    }
    if (c.right_precond != (right == 1)) {
        hipStreamSynchronize(c.stream);
        iter_graphs_clear(c);  // captured for the other variant
        c.right_precond = right == 1;
    }
    return 0;
}

int fedm_set_fieldsplit_order(fedm_ctx *h, int upper) {
    Ctx &c = h->c;
    if (upper != 0 && upper != 1) {
        set_error("field-split order must be 0 (lower) or 1 (upper)");
        return -2;
    }
    if (c.fs_upper != (upper == 1)) {
        hipStreamSynchronize(c.stream);
        iter_graphs_clear(c);  // captured for the other order
        c.fs_upper = upper == 1;
    }
    return 0;
}

int fedm_set_krylov_scaling(fedm_ctx *h, int mode) {
    if (!h) return -2;
    Ctx &c = h->c;
    if (mode != 0 && mode != 1) {
        set_error("krylov scaling mode must be 0 (none) or 1 (rows)");
        return -2;
    }
    if (c.krylov_scaling != mode) {
        FEDM_HIP_CHECK(hipSetDevice(c.device));
        hipStreamSynchronize(c.stream);
        iter_graphs_clear(c);  // captured with the other instantiations of the reduction kernels
        if (mode == 1 && !c.d_kscale2) FEDM_HIP_CHECK(hipMalloc((void **)&c.d_kscale2, sizeof(double) * c.np));
        c.krylov_scaling = mode;
    }
    return 0;
}

int fedm_get_krylov_scaling(fedm_ctx *h, int *mode, double *d_out) {
    if (!h) return -2;
    Ctx &c = h->c;
    if (mode) *mode = c.krylov_scaling;
    if (!d_out) return 0;
    FEDM_HIP_CHECK(hipSetDevice(c.device));
    // from the Jacobian as it stands: what a scaled solve started now would use (d^2 goes to scratch when no scaled
    // solve has run on this context)
    launch_row_scale(c, c.d_kscale2 ? c.d_kscale2 : c.d_tmp, c.d_w);
    return get_vec(c, d_out, c.d_w);
}

int fedm_plane_masks(fedm_ctx *h, uint32_t *kept_planes, uint32_t *zero_planes) {
    Ctx &c = h->c;
    if (kept_planes) *kept_planes = (c.skip_const_planes && c.assembly_kind == 1 && c.assembly_lean >= 2) ? c.const_plane_mask : 0u;
    if (zero_planes) *zero_planes = c.neq == 3 ? (c.zero_plane_mask & 10u) : 0u;
    return 0;
}

int fedm_sizes(fedm_ctx *h, int64_t *n_vertices, int64_t *n_cells, int64_t *n_eq,
               int64_t *nnz_blocks, int64_t *stored_blocks, int64_t *n_colours) {
    Ctx &c = h->c;
    if (n_vertices) *n_vertices = c.nv;
    if (n_cells) *n_cells = c.nc;
    if (n_eq) *n_eq = c.neq;
    if (nnz_blocks) *nnz_blocks = c.pat.nnz_blocks;
    if (stored_blocks) *stored_blocks = c.pat.total_bc * SLICE;
    if (n_colours) *n_colours = (int64_t)c.pat.colour_ptr.size() - 1;
    return 0;
}

int fedm_pattern_info(fedm_ctx *h, int64_t out[9]) {
    if (!h || !out) return -2;
    Ctx &c = h->c;
    out[0] = c.pat.n_slices;
    out[1] = c.pat.max_patch_cells;
    out[2] = c.pat.max_patch_width;
    out[3] = c.pat.max_patch_verts;
    out[4] = (int64_t)c.pat.patch_cells.size();
    out[5] = (int64_t)c.pat.patch_halo.size();
    // the volume assembly the next fedm_jacobian call runs (assemble.hip, assembly_path: the dispatch's own
    // decision): 0 global colouring, 1 LDS patches with the unrolled element routine, 2 LDS patches one equation
    // row at a time (lean2 kernels), 3 LDS patches, one pass over the cells (lean3 kernels, assemble3.hip)
    const AssemblyPath path = assembly_path(c, true, 0);
    const int variant = path.variant;
    out[6] = variant < 0 ? 0 : variant;
    out[7] = path.threads;
    // the one-pass kernels with the model's structure compiled in (assemble3.hip, Lean3SigBenchmark)
    out[8] = variant == 3 ? lean3_signature(c) : 0;
    return 0;
}

}  // extern "C"
