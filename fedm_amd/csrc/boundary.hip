// What runs behind the volume assembly (assemble.hip): the Neumann and wall facets, the Dirichlet rows, the identity
// rows of ghost, padding and frozen-species dofs, and the launch that takes facets and rows together.
#include <cassert>
#include <type_traits>

#include "dielectric.hpp"
#include "element.hpp"
#include "fedm_internal.hpp"

namespace fedm {

// =============================================================================================
// Neumann boundary facets (fedm/functions.py:523-524): one thread per tagged facet, one launch
// per facet colour (facets of a colour share no vertex), plain adds on top of the volume
// assembly -> fixed summation order.
// =============================================================================================

// Where boundary_facet's terms go: the residual entry (vertex a, component s) and the entry (sr, scol) of the cell's
// block (a, b), found through cell_slots.  ATOMIC: fp64 atomics (all facets in one launch) or plain adds (one colour).
// SPECIES_COLS: the species columns only (the segregated step's species assembly leaves the potential column's planes).
// The members refer to the kernel's own variables, as a [&] lambda's captures do: with copies 26 facet kernels change.
template <int NEQ, bool ATOMIC>
struct ResidualSink {
    double *__restrict__ &F;
    int (&v)[3];
    __device__ __forceinline__ void operator()(int a, int s, double value) const {
        double *p = &F[(size_t)v[a] * NEQ + s];
        if (ATOMIC) unsafeAtomicAdd(p, value);
        else *p += value;
    }
};
template <int NEQ, bool ATOMIC, bool SPECIES_COLS>
struct JacobianSink {
    double *__restrict__ &val;
    const uint32_t *__restrict__ &cell_slots;
    const int &c;
    __device__ __forceinline__ void operator()(int a, int b, int sr, int scol, double value) const {
        if (SPECIES_COLS && scol == NEQ - 1) return;
        const uint32_t slot = cell_slots[(size_t)c * 9 + a * 3 + b];
        double *p = &val[((size_t)(slot >> 6) * NEQ * NEQ + sr * NEQ + scol) * SLICE + (slot & 63)];
        if (ATOMIC) unsafeAtomicAdd(p, value);
        else *p += value;
    }
};

// A facet of a dielectric layer (dielectric.hpp): q_a(u) of the Poisson row is dt (1 + w)/(1 + 2w) e sum_s Z_s W_a,s(u)
// plus history, W_a,s being exactly what goes through the sinks above for species row s.  So every residual term
// (a, s, v) goes once more to (a, Phi, -kappa Z_s v) and every Jacobian entry (a, b, s, col, v) to (a, b, Phi, col,
// -kappa Z_s v), the potential column included: the mirror is made here, where the terms are placed, and the wall
// formulas of element.hpp stay the one copy.  Facets of other tags pass through unchanged.
template <int NS, bool TAB, bool WALL, class AddR, class AddJ>
__device__ __forceinline__ void mirrored_facet(const fedm_model_desc *__restrict__ md, const double x[3][2],
                                               const double Uc[3][NS + 1], int fi, int tag, bool jacobian, AddR addR,
                                               AddJ addJ, const LayerMirror &lm) {
    const bool on = (lm.tags >> (tag - 1)) & 1u;
    auto mirrorR = [&](int a, int s, double value) {
        addR(a, s, value);
        if (on) addR(a, NS, lm.kz[s] * value);
    };
    auto mirrorJ = [&](int a, int b, int sr, int scol, double value) {
        addJ(a, b, sr, scol, value);
        if (on) addJ(a, b, NS, scol, lm.kz[sr] * value);
    };
    boundary_facet<NS, TAB, WALL>(md, x, Uc, fi, tag, jacobian, mirrorR, mirrorJ);
}

// The facet record and the gather of its cell stand in both facet kernels, not in a helper: a device function that does
// them is optimised on its own, with generic pointers, before it is inlined, and kernels come out with other registers,
// scratch or spills than before the split (profiles/boundary_split_resources.md).
// WALL: the 'flux source' wall terms besides (element.hpp, wall_facet; Ctx::model_walls)
// Layer: empty, or -- the DIEL switch, for a model with dielectric layers (Ctx::diel) -- one LayerMirror, which the
// kernel then takes as its last argument.  A pack, so that without it the kernel has the signature and the body it had.
template <int NS, bool ATOMIC, bool SPECIES_COLS = false, bool TAB = false, bool WALL = false, class... Layer>
__global__ void boundary_kernel(const fedm_model_desc *__restrict__ md, int n_facets,
                                const int *__restrict__ facets /* [n][3] = cell, local facet, tag */,
                                const int *__restrict__ cells, const double *__restrict__ coords,
                                const uint32_t *__restrict__ cell_slots,
                                const double *__restrict__ u, double *__restrict__ val,
                                double *__restrict__ F, int jacobian, Layer... layer) {
    static_assert(sizeof...(Layer) <= 1 && !(SPECIES_COLS && sizeof...(Layer)), "one LayerMirror, full assembly only");
    constexpr int NEQ = NS + 1;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_facets) return;
    const int c = facets[3 * t], fi = facets[3 * t + 1], tag = facets[3 * t + 2];
    int v[3];
    double x[3][2], Uc[3][NEQ];
    for (int a = 0; a < 3; ++a) {
        v[a] = cells[3 * c + a];
        x[a][0] = coords[2 * v[a]];
        x[a][1] = coords[2 * v[a] + 1];
        for (int s = 0; s < NEQ; ++s) Uc[a][s] = u[(size_t)v[a] * NEQ + s];
    }
    ResidualSink<NEQ, ATOMIC> addR{F, v};
    JacobianSink<NEQ, ATOMIC, SPECIES_COLS> addJ{val, cell_slots, c};
    if constexpr (sizeof...(Layer) == 0) boundary_facet<NS, TAB, WALL>(md, x, Uc, fi, tag, jacobian != 0, addR, addJ);
    else mirrored_facet<NS, TAB, WALL>(md, x, Uc, fi, tag, jacobian != 0, addR, addJ, layer...);
}

// The model's compile-time switches from its run-time flags: fn(NS, TAB, WALL, DIEL) with std::integral_constants for
// (c.ns, c.model_tables, c.model_walls, c.diel != null) -- the one place that turns them into template arguments of the
// kernels here
template <class Fn>
static void with_model_flags(const Ctx &c, Fn &&fn) {
    auto layers = [&](auto ns, auto tab, auto wall) {
        if (c.diel) fn(ns, tab, wall, std::true_type{});
        else fn(ns, tab, wall, std::false_type{});
    };
    auto flags = [&](auto ns) {
        if (c.model_walls && c.model_tables) layers(ns, std::true_type{}, std::true_type{});
        else if (c.model_walls) layers(ns, std::false_type{}, std::true_type{});
        else if (c.model_tables) layers(ns, std::true_type{}, std::false_type{});
        else layers(ns, std::false_type{}, std::false_type{});
    };
    switch (c.ns) {
        case 1: flags(std::integral_constant<int, 1>{}); break;
        case 2: flags(std::integral_constant<int, 2>{}); break;
        case 3: flags(std::integral_constant<int, 3>{}); break;
        case 4: flags(std::integral_constant<int, 4>{}); break;
    }
}

template <bool ATOMIC>
static void launch_boundary_range(Ctx &c, bool jacobian, int f0, int n) {
    const dim3 g((n + 127) / 128), b(128);
    const int *fl = c.d_bfacets + 3 * f0;
    with_model_flags(c, [&](auto ns, auto tab, auto wall, auto diel) {
        constexpr int NS = decltype(ns)::value;
        constexpr bool TAB = decltype(tab)::value, WALL = decltype(wall)::value;
        if constexpr (decltype(diel)::value)
            hipLaunchKernelGGL((boundary_kernel<NS, ATOMIC, false, TAB, WALL, LayerMirror>), g, b, 0, c.stream, c.d_model, n,
                               fl, c.d_cells, c.d_coords, c.d_cell_slots, c.d_u, c.d_val, c.d_F, jacobian ? 1 : 0,
                               layer_mirror(c));
        else
            hipLaunchKernelGGL((boundary_kernel<NS, ATOMIC, false, TAB, WALL>), g, b, 0, c.stream, c.d_model, n, fl,
                               c.d_cells, c.d_coords, c.d_cell_slots, c.d_u, c.d_val, c.d_F, jacobian ? 1 : 0);
    });
}

void launch_boundary(Ctx &c, bool jacobian) {
    if (!c.poisson || c.n_bfacets == 0) return;
    if (c.assembly_kind == 1) {
        // the patch assembly already sums in a run-dependent order (LDS atomics): all facets in
        // one launch with fp64 atomics instead of one launch per colour
        launch_boundary_range<true>(c, jacobian, 0, c.n_bfacets);
        return;
    }
    const int ncol = (int)c.bfacet_colour_ptr.size() - 1;
    for (int k = 0; k < ncol; ++k) {
        const int f0 = c.bfacet_colour_ptr[k], n = c.bfacet_colour_ptr[k + 1] - f0;
        if (n > 0) launch_boundary_range<false>(c, jacobian, f0, n);
    }
}

// The facets behind the species-only one-pass kernel (launch_assemble_species): one launch with atomics, the species
// columns only.  Instantiated, like that kernel, for two species without tables or walls (assemble3.hip, lean3_applies).
void launch_boundary_species_cols(Ctx &c, bool jacobian) {
    if (c.n_bfacets == 0) return;
    assert(c.ns == 2 && !c.model_tables && !c.model_walls && !c.diel);
    const dim3 g((c.n_bfacets + 127) / 128), b(128);
    with_model_flags(c, [&](auto ns, auto tab, auto wall, auto diel) {
        if constexpr (decltype(ns)::value == 2 && !decltype(tab)::value && !decltype(wall)::value && !decltype(diel)::value)
            hipLaunchKernelGGL((boundary_kernel<2, true, true>), g, b, 0, c.stream, c.d_model, c.n_bfacets, c.d_bfacets,
                               c.d_cells, c.d_coords, c.d_cell_slots, c.d_u, c.d_val, c.d_F, jacobian ? 1 : 0);
    });
}

// =============================================================================================
// Dirichlet rows (bc.apply(b, x): b_i = x_i - g_i; bc.apply(A): identity row), padding
// vertices and -- in Poisson-only mode -- frozen species rows.
// =============================================================================================

// The unit row of component cr of vertex vtx: zero in every block column of the vertex's slice, 1 on the diagonal.
// (padded duplicates of the diagonal column stay zero: diag_slot names the first match)
__device__ __forceinline__ void unit_row(double *__restrict__ val, const int *__restrict__ boff,
                                         const uint32_t *__restrict__ diag_slot, int neq, int vtx, int cr) {
    const int neq2 = neq * neq;
    const int slice = vtx >> 6, lane = vtx & 63;
    for (int bc = boff[slice]; bc < boff[slice + 1]; ++bc)
        for (int cc = 0; cc < neq; ++cc)
            val[((size_t)bc * neq2 + cr * neq + cc) * SLICE + lane] = 0.0;
    const uint32_t ds = diag_slot[vtx];
    val[((size_t)(ds >> 6) * neq2 + cr * neq + cr) * SLICE + (ds & 63)] = 1.0;
}

// Dirichlet rows (F = u - value, unit row) and, in the same launch when no species is frozen, the
// identity rows of the vertices [n_owned, nvp) (ghosts and padding): one kernel boundary less per
// assembly.  n_id = 0: Dirichlet rows only.
__global__ void dirichlet_kernel(int n_dir, const int *__restrict__ dofs,
                                 const double *__restrict__ vals, const double *__restrict__ u,
                                 double *__restrict__ F, double *__restrict__ val,
                                 const int *__restrict__ boff, const int *__restrict__ colidx,
                                 const uint32_t *__restrict__ diag_slot, int neq, int jacobian,
                                 int id_first, int n_id, const int *__restrict__ id_list, int n_list) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_dir) {
        if (t - n_dir >= n_id) return;
        // identity rows: the range [id_first, ...) or, with deep halos, the listed ghost vertices (the
        // outermost layer) followed by the padding range
        const int k = t - n_dir;
        const int vtx = id_list ? (k < n_list ? id_list[k] : id_first + (k - n_list)) : id_first + k;
        for (int cr = 0; cr < neq; ++cr) {
            F[(size_t)vtx * neq + cr] = 0.0;
            if (jacobian) unit_row(val, boff, diag_slot, neq, vtx, cr);
        }
        return;
    }
    const int dof = dofs[t];
    const int vtx = dof / neq, cr = dof % neq;
    // (n_dir counts the Dirichlet ROWS, Ctx::n_dir_rows: a dof of a vertex with identity rows is not among them;
    // on an assembled ghost row of a deep halo the Dirichlet condition applies as on its owner)
    F[dof] = u[dof] - vals[t];
    if (jacobian) unit_row(val, boff, diag_slot, neq, vtx, cr);
}

// rows that are identity by construction: padding vertices (all components) and, in
// Poisson-only mode, every species component of every vertex
__global__ void identity_rows_kernel(int nv, int nvp, int neq, int ns_frozen,
                                     double *__restrict__ F, double *__restrict__ val,
                                     const int *__restrict__ boff,
                                     const uint32_t *__restrict__ diag_slot, int jacobian) {
    const int vtx = blockIdx.x * blockDim.x + threadIdx.x;
    if (vtx >= nvp) return;
    const int n_rows = (vtx >= nv) ? neq : ns_frozen;
    for (int cr = 0; cr < n_rows; ++cr) {
        F[(size_t)vtx * neq + cr] = 0.0;
        if (jacobian) unit_row(val, boff, diag_slot, neq, vtx, cr);
    }
}

// boundary_kernel<NS, true> and dirichlet_kernel in one launch (128-thread blocks: the first ones take the facets, the
// rest the Dirichlet and padding rows) -- allowed when no row belongs to both (Ctx::boundary_rows_disjoint)
// Layer: as boundary_kernel's
template <int NS, bool TAB, bool WALL = false, class... Layer>
__global__ __launch_bounds__(128) void boundary_dirichlet_kernel(
    const fedm_model_desc *__restrict__ md, int n_facets, int facet_blocks, const int *__restrict__ facets,
    const int *__restrict__ cells, const double *__restrict__ coords, const uint32_t *__restrict__ cell_slots,
    const double *__restrict__ u, double *__restrict__ val, double *__restrict__ F, int jacobian, int n_dir,
    const int *__restrict__ dofs, const double *__restrict__ vals, const int *__restrict__ boff,
    const uint32_t *__restrict__ diag_slot, int id_first, int n_id, Layer... layer) {
    static_assert(sizeof...(Layer) <= 1, "one LayerMirror");
    constexpr int NEQ = NS + 1;
    if ((int)blockIdx.x < facet_blocks) {
        const int t = blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= n_facets) return;
        const int c = facets[3 * t], fi = facets[3 * t + 1], tag = facets[3 * t + 2];
        int v[3];
        double x[3][2], Uc[3][NEQ];
        for (int a = 0; a < 3; ++a) {
            v[a] = cells[3 * c + a];
            x[a][0] = coords[2 * v[a]];
            x[a][1] = coords[2 * v[a] + 1];
            for (int s = 0; s < NEQ; ++s) Uc[a][s] = u[(size_t)v[a] * NEQ + s];
        }
        ResidualSink<NEQ, true> addR{F, v};
        JacobianSink<NEQ, true, false> addJ{val, cell_slots, c};
        if constexpr (sizeof...(Layer) == 0) boundary_facet<NS, TAB, WALL>(md, x, Uc, fi, tag, jacobian != 0, addR, addJ);
        else mirrored_facet<NS, TAB, WALL>(md, x, Uc, fi, tag, jacobian != 0, addR, addJ, layer...);
        return;
    }
    // the rows of dirichlet_kernel (one GPU: Dirichlet dofs, then the padding vertices [id_first, id_first + n_id))
    const int t = ((int)blockIdx.x - facet_blocks) * blockDim.x + threadIdx.x;
    if (t >= n_dir + n_id) return;
    if (t >= n_dir) {
        const int vtx = id_first + (t - n_dir);
        for (int cr = 0; cr < NEQ; ++cr) {
            F[(size_t)vtx * NEQ + cr] = 0.0;
            if (jacobian) unit_row(val, boff, diag_slot, NEQ, vtx, cr);
        }
        return;
    }
    const int dof = dofs[t], vtx = dof / NEQ, cr = dof % NEQ;
    F[dof] = u[dof] - vals[t];
    if (jacobian) unit_row(val, boff, diag_slot, NEQ, vtx, cr);
}

void launch_finalize(Ctx &c, bool jacobian, int mode) {
    if (c.boundary_pending) {
        const bool jac = c.boundary_pending == 2;
        c.boundary_pending = 0;
        if (mode == 0 && jac == jacobian) {
            const int fb = (c.n_bfacets + 127) / 128, n_id = c.nvp - c.nv;
            const int rb = (c.n_dir_rows + n_id + 127) / 128;   // (no identity vertices here: n_dir_rows == n_dir)
            with_model_flags(c, [&](auto ns, auto tab, auto wall, auto diel) {
                constexpr int NS = decltype(ns)::value;
                constexpr bool TAB = decltype(tab)::value, WALL = decltype(wall)::value;
                if constexpr (decltype(diel)::value)
                    hipLaunchKernelGGL((boundary_dirichlet_kernel<NS, TAB, WALL, LayerMirror>), dim3(fb + rb), dim3(128), 0,
                                       c.stream, c.d_model, c.n_bfacets, fb, c.d_bfacets, c.d_cells, c.d_coords,
                                       c.d_cell_slots, c.d_u, c.d_val, c.d_F, jacobian ? 1 : 0, c.n_dir_rows, c.d_dir_dofs,
                                       c.d_dir_vals, c.d_slice_boff, c.d_diag_slot, c.nv, n_id, layer_mirror(c));
                else
                    hipLaunchKernelGGL((boundary_dirichlet_kernel<NS, TAB, WALL>), dim3(fb + rb), dim3(128), 0, c.stream,
                                       c.d_model, c.n_bfacets, fb, c.d_bfacets, c.d_cells, c.d_coords, c.d_cell_slots, c.d_u,
                                       c.d_val, c.d_F, jacobian ? 1 : 0, c.n_dir_rows, c.d_dir_dofs, c.d_dir_vals,
                                       c.d_slice_boff, c.d_diag_slot, c.nv, n_id);
            });
            return;
        }
        launch_boundary(c, jac);   // (not the pair this was deferred for: the facets first, then the rows as usual)
    }
    const int ns_frozen = (mode == 1) ? c.ns : 0;
    const bool deep = c.d_identity != nullptr;
    // identity rows: padding + ghost vertices (deep halos: padding + the listed outermost ghost layer)
    int n_id = deep ? c.n_identity + (c.nvp - c.nv) : c.nvp - c.n_owned;
    if (ns_frozen > 0) {           // frozen species: every vertex has identity rows
        // (vertices beyond the first argument: all rows -- the ghosts of a one-layer halo and the padding;
        // deep halos: the padding only, the inner ghost layers keep their potential rows and the
        // outermost layer is listed)
        hipLaunchKernelGGL(identity_rows_kernel, dim3((c.nvp + 255) / 256), dim3(256), 0, c.stream,
                           deep ? c.nv : c.n_owned, c.nvp, c.neq, ns_frozen, c.d_F, c.d_val, c.d_slice_boff,
                           c.d_diag_slot, jacobian ? 1 : 0);
        n_id = deep ? c.n_identity : 0;
    }
    // (Dirichlet dofs of vertices with identity rows -- one-layer ghosts, the listed layer of a deep halo -- stand
    // behind the first n_dir_rows entries of the list and are left to the identity branch: the row sets are disjoint)
    if (c.n_dir_rows + n_id > 0)
        hipLaunchKernelGGL(dirichlet_kernel, dim3((c.n_dir_rows + n_id + 255) / 256), dim3(256), 0, c.stream,
                           c.n_dir_rows, c.d_dir_dofs, c.d_dir_vals, c.d_u, c.d_F, c.d_val,
                           c.d_slice_boff, c.d_colidx, c.d_diag_slot, c.neq, jacobian ? 1 : 0,
                           deep ? c.nv : c.n_owned, n_id, c.d_identity, c.n_identity);
}

__global__ void set_dirichlet_state_kernel(int n_dir, const int *__restrict__ dofs,
                                           const double *__restrict__ vals, double *__restrict__ u) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_dir) u[dofs[t]] = vals[t];
}

void launch_set_dirichlet_state(Ctx &c) {
    if (c.n_dir > 0)
        hipLaunchKernelGGL(set_dirichlet_state_kernel, dim3((c.n_dir + 255) / 256), dim3(256), 0,
                           c.stream, c.n_dir, c.d_dir_dofs, c.d_dir_vals, c.d_u);
}

}  // namespace fedm
