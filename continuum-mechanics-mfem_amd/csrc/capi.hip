// capi.hip — the C-ABI of libcdfem.so (include/cdfem.h): context, mesh/space upload, partial and full
// assembly setup, FormLinearSystem, the entry to the Krylov solves, profiling.  Host-side orchestration
// only: the Krylov drivers are in solve.hip, the option table in options.hpp, the cost model in model.hip,
// and all arithmetic on the hot path runs in the HIP kernels (pa_kernels.hip, vec_kernels.hip, ...).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "cdfem_internal.hpp"
#include "host_util.hpp"
#include "brick_core.hpp"

using namespace cdfem;

// ---- the raw resources behind the handles (handles.hpp) -----------------------------------------
void *cdfem::raw_device_alloc(size_t bytes)
{
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    return p;
}
void cdfem::raw_device_free(void *p) noexcept { (void)hipFree(p); }
void *cdfem::raw_pinned_alloc(size_t bytes)
{
    void *p = nullptr;
    HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    return p;
}
void cdfem::raw_pinned_free(void *p) noexcept { (void)hipHostFree(p); }
hipEvent_t cdfem::raw_event_create(bool timing)
{
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming));
    return e;
}
void cdfem::raw_event_destroy(hipEvent_t e) noexcept { (void)hipEventDestroy(e); }

// ---- profiling helpers ---------------------------------------------------------------------------
void cdfem::prof_mark(cdfem_ctx *c, int k, bool begin)
{
    if (!c->profile || !((c->prof_mask >> k) & 1u)) return;
    ProfileSlot &s = c->prof[k];
    const size_t need = (size_t)(s.used + 1) * 2;
    while (s.ev.size() < need) s.ev.emplace_back().create(true);
    if (begin) {
        // recorded now AND armed: a CDFEM_LAUNCH before the end mark re-records the pair tightly
        // around its own dispatch; any other launch leaves the plain event interval
        HIPCHK(hipEventRecord(s.ev[2 * s.used], c->stream));
        c->ext_ev[0] = s.ev[2 * s.used];
        c->ext_ev[1] = s.ev[2 * s.used + 1];
    } else {
        if (c->ext_ev[0]) HIPCHK(hipEventRecord(s.ev[2 * s.used + 1], c->stream));  // not consumed
        c->ext_ev[0] = c->ext_ev[1] = nullptr;
        s.used++;
    }
}

void cdfem::prof_collect(cdfem_ctx *c)
{
    if (!c->profile) return;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &s : c->prof) {
        for (int i = 0; i < s.used; ++i) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, s.ev[2 * i], s.ev[2 * i + 1]));
            s.total_ms += ms;
            s.count++;
            s.each.push_back(ms);
        }
        s.used = 0;
    }
}

namespace {

// every element a parallelepiped: each vertex v (lexicographic, bit k = axis k) equals
// v0 + sum_k bit_k (v_{2^k} - v0) up to the rounding of those coordinates (32 ulp of the largest
// coordinate magnitude) plus 1e-12 of the element's longest edge.  Then the multilinear map is
// affine and its Jacobian is the edge matrix at every point (the PA setup's pa_affine form) to a
// relative 1e-12 of the element (the tolerance was 1e-13 of max(|x|, edge), which for
// small elements far from the origin admitted defects far larger than the element's own scale).
static bool mesh_is_affine(int dim, int64_t ne, const double *V)
{
    const int nv = 1 << dim;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int64_t e = 0; e < ne; ++e) {
        const double *X = V + (size_t)e * nv * dim;
        double xmax = 0.0, hmax = 0.0;
        for (int v = 0; v < nv; ++v)
            for (int i = 0; i < dim; ++i) xmax = std::max(xmax, std::fabs(X[v * dim + i]));
        for (int k = 0; k < dim; ++k) {
            double h2 = 0.0;
            for (int i = 0; i < dim; ++i) {
                const double d = X[(1 << k) * dim + i] - X[i];
                h2 += d * d;
            }
            hmax = std::max(hmax, std::sqrt(h2));
        }
        const double tol = 32.0 * eps * xmax + 1e-12 * hmax;
        for (int v = 3; v < nv; ++v) {
            if ((v & (v - 1)) == 0) continue;  // the edge vertices themselves
            for (int i = 0; i < dim; ++i) {
                double p = X[i];
                for (int k = 0; k < dim; ++k)
                    if (v >> k & 1) p += X[(1 << k) * dim + i] - X[i];
                if (std::fabs(p - X[v * dim + i]) > tol) return false;
            }
        }
    }
    return true;
}

// a new mesh starts from nothing: every buffer of the old one freed, every flag at its initialiser
void free_mesh(cdfem_ctx *c)
{
    ilu_free(c);
    partition_free(c);
    static_cast<MeshState &>(*c) = MeshState{};
}

// per brick (edge E elements in x and y, EZ in z; nb* bricks per axis): 1 if a lattice dof of its patch
// (E p + 1 per axis, EZ p + 1 along z, clipped to the lattice) is essential; the brick CG kernels skip the
// essential-flag loads elsewhere
static void upload_brick_ess(cdfem_ctx *c, int E, int EZ, int nbx, int nby, int nbz)
{
    const int64_t s1 = (int64_t)E * c->p, sz1 = (int64_t)EZ * c->p, Lx = c->Lx, Ly = c->Ly, Lz = c->Lz;
    std::vector<uint8_t> has((size_t)nbx * nby * nbz, 0);
    for (int bz = 0; bz < nbz; ++bz)
        for (int by = 0; by < nby; ++by)
            for (int bx = 0; bx < nbx; ++bx) {
                uint8_t h = 0;
                for (int64_t z = bz * sz1; z <= std::min(bz * sz1 + sz1, Lz - 1) && !h; ++z)
                    for (int64_t y = by * s1; y <= std::min(by * s1 + s1, Ly - 1) && !h; ++y) {
                        const uint8_t *row = c->h_ess.data() + (size_t)(z * Ly + y) * Lx;
                        for (int64_t x = bx * s1; x <= std::min(bx * s1 + s1, Lx - 1); ++x) h |= row[x];
                    }
                has[((size_t)bz * nby + by) * nbx + bx] = h;
            }
    c->d_bess.alloc(has.size());
    HIPCHK(hipMemcpy(c->d_bess, has.data(), has.size(), hipMemcpyHostToDevice));
}

// (Re)build the element-block layout for a permutation perm[blk*64 + lane] = element (-1 pad):
// element map [blk][l][lane] (ess negative), E->L positions, and the device permutation.
void build_layout(cdfem_ctx *c, const std::vector<int32_t> &perm)
{
    const int nd = c->nd;
    const int64_t nl = c->nl;
    std::vector<int32_t> map((size_t)c->nblk * nd * kLanes, 0);
    std::vector<int32_t> where(c->ne, -1);
    for (size_t k = 0; k < perm.size(); ++k)
        if (perm[k] >= 0) where[perm[k]] = (int32_t)k;
    // E-vector / map index of (element, local dof): blocks of 64 lanes, or element-major
    auto eidx = [&](int e, int l) -> size_t {
        if (c->qlay == 1) return (size_t)e * nd + l;
        const int blk = where[e] / kLanes, lane = where[e] % kLanes;
        return ((size_t)blk * nd + l) * kLanes + lane;
    };
    std::vector<int32_t> cnt(nl + 1, 0);
    for (int e = 0; e < c->ne; ++e) {
        for (int l = 0; l < nd; ++l) {
            const int32_t g = c->h_dofs[(size_t)e * nd + l];
            map[eidx(e, l)] = c->h_ess[g] ? -(g + 1) : g;
            cnt[g + 1]++;
        }
    }
    for (int64_t i = 0; i < nl; ++i) cnt[i + 1] += cnt[i];
    std::vector<int32_t> pos((size_t)c->ne * nd), fill(cnt.begin(), cnt.end() - 1);
    for (int e = 0; e < c->ne; ++e) {
        for (int l = 0; l < nd; ++l) {
            const int32_t g = c->h_dofs[(size_t)e * nd + l];
            pos[fill[g]++] = (int32_t)eidx(e, l);
        }
    }
    upload(c, c->d_map, map);
    upload(c, c->d_e2l_off, cnt);
    upload(c, c->d_e2l_pos, pos);
    upload(c, c->d_perm, perm);
    c->d_Ye.alloc((size_t)c->nblk * nd * kLanes);
    c->d_part.alloc((size_t)c->red_blocks + c->nblk + 64 * 8192 + 16384);
    HIPCHK(hipMemsetAsync(c->d_Ye, 0, (size_t)c->nblk * nd * kLanes * sizeof(double), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

}  // namespace

// ---- call-order checks and the copy-in / copy-out helpers of the entry points (host_util.hpp) ----
namespace cdfem {

void require_mesh(cdfem_ctx *c)
{
    if (!c->mesh_ready) throw StateError("cdfem_mesh_upload has not been called");
}
void require_pa(cdfem_ctx *c)
{
    require_mesh(c);
    if (!c->pa_ready && !c->fa_ready && !nl_jac_current(c))
        throw StateError("no operator: call cdfem_pa_setup or cdfem_fa_setup");
}

// a communicator of more than one rank needs a declared partition: the z-slab of a structured box
// (cdfem_set_slab) or the general shared-dof lists (cdfem_set_shared).  Without one, the exchange
// would read unset interface buffers and the ranks would take different Krylov branches.
void require_partition(cdfem_ctx *c)
{
    if (!multi_rank(c)) return;
    if (c->part_mode == 1) {
        if (!c->structured || !c->d_if[0]) throw StateError("slab partition incomplete: cdfem_set_slab after cdfem_mesh_set_structured");
        if (c->fa_ready) throw UnsupportedError("slab partitions drive partial-assembly operators; use cdfem_set_shared for assembled ones");
        return;
    }
    if (c->part_mode == 2) {
        if (use_brick(c)) throw UnsupportedError("the structured brick kernels need a slab partition (cdfem_set_slab)");
        return;
    }
    throw StateError("communicator attached (" + std::to_string(c->nranks) +
                     " ranks) but no partition declared: call cdfem_set_slab or cdfem_set_shared");
}

// copy-in helper: returns a device pointer holding n doubles of src (staging when on host)
const double *dev_in(cdfem_ctx *c, const double *src, int where, double *staging, size_t n)
{
    if (where == CDFEM_DEVICE) return src;
    HIPCHK(hipMemcpyAsync(staging, src, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return staging;
}

void dev_out(cdfem_ctx *c, double *dst, int where, const double *dsrc, size_t n)
{
    if (where == CDFEM_DEVICE) {
        if (dst != dsrc)
            HIPCHK(hipMemcpyAsync(dst, dsrc, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return;
    }
    HIPCHK(hipMemcpyAsync(dst, dsrc, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

// the assembled operator's CSR pattern, contribution lists and SELL copy on the device: once per mesh
void fa_ensure_pattern(cdfem_ctx *c)
{
    if (c->d_rowptr) return;
    // a multi-rank partition keeps the mesh order (its shared-dof exchange indexes L-vectors)
    // dof coordinates for the geometric SpMV order (simplex geometry is on the host; quads and hexes keep
    // theirs on the device alone, read back here once per mesh)
    std::vector<double> xyz;
    if (!multi_rank(c) && (c->sell_mode == 3 || c->sell_mode >= 5)) {
        if (c->geom == 0) {
            std::vector<double> verts((size_t)c->ne * c->nv * c->dim);
            HIPCHK(hipMemcpy(verts.data(), c->d_verts, verts.size() * sizeof(double), hipMemcpyDeviceToHost));
            xyz = tensor_dof_coords(c->dim, c->p, c->ne, c->nd, c->nl, verts, c->h_dofs);
        } else if (!c->h_verts.empty()) {
            xyz = simplex_dof_coords(c->dim, c->p, c->ne, c->nd, c->nl, c->h_verts, c->h_dofs);
        }
    }
    FaPattern P = fa_build_pattern(c->h_dofs, c->ne, c->nd, c->nl,
                                   multi_rank(c) ? 0 : c->sell_mode, c->dim,
                                   xyz.empty() ? nullptr : xyz.data(), c->sell_window, c->spmv_lds,
                                   c->spmv_lpr);
    if (P.lds_rows > 0) {
        // the LDS-staged SpMV launches one block per window (rounded up to whole XCD ranges)
        // and its CG form writes one partial per block: the grid must fit the partial slots
        // (ADVICE r03).  Windows halve below their nominal size when halos are large, so the
        // automatic choice falls back to the layout without LDS; an explicit one is refused.
        const int64_t spw = P.lds_rows / (kLanes / std::max(1, P.lpr));
        const int64_t nwin = ((int64_t)P.sptr.size() - 1 + spw - 1) / spw;
        if (8 * ((nwin + 7) / 8) > kSpmvMaxBlocks) {
            if (c->spmv_lds >= 0)
                throw UnsupportedError("spmv_lds " + std::to_string(c->spmv_lds) + ": " +
                                       std::to_string(nwin) + " LDS windows exceed the SpMV grid (" +
                                       std::to_string(kSpmvMaxBlocks) + " blocks); use larger windows or 0");
            P = fa_build_pattern(c->h_dofs, c->ne, c->nd, c->nl, multi_rank(c) ? 0 : c->sell_mode,
                                 c->dim, xyz.empty() ? nullptr : xyz.data(), c->sell_window, 0, 1);
        }
    }
    const int64_t nslices = (int64_t)P.sptr.size() - 1;
    if ((nslices + 3) / 4 + 8 > kSpmvMaxBlocks) throw UnsupportedError("matrix too large for the SpMV grid");
    // built aside and moved into the context whole, after the last call that can throw
    FaDeviceState F;
    F.nnz = P.nnz;
    upload(c, F.d_rowptr, P.rowptr);
    upload(c, F.d_cols, P.cols);
    upload(c, F.d_diagpos, P.diagpos);
    upload(c, F.d_coff, P.coff);
    upload(c, F.d_cpos, P.cpos);
    F.d_vals.alloc(F.nnz);
    F.d_vals_c.alloc(F.nnz);
    F.d_Ee.alloc((size_t)c->nblk * c->nd * c->nd * kLanes);
    F.nslices = nslices;
    F.nstored = P.sptr.back();
    upload(c, F.d_sptr, P.sptr);
    upload(c, F.d_srows, P.srows);
    upload(c, F.d_scols, P.scols);
    upload(c, F.d_smap, P.smap);
    F.d_svals.alloc(F.nstored);
    F.d_svals_c.alloc(F.nstored);
    F.sell_windowed = P.windowed;
    if (!P.perm.empty()) {
        upload(c, F.d_rperm, P.perm);
        for (auto &v : F.d_pv) v.alloc(c->nl);
    }
    if (!P.sdel.empty()) upload(c, F.d_sdel, P.sdel);
    if (P.lds_rows > 0) {  // LDS-staged windows (sell_plan.cpp)
        upload(c, F.d_hptr, P.hptr);
        upload(c, F.d_hidx, P.hidx);
        upload(c, F.d_sloc, P.sloc);
        F.lds_rows = P.lds_rows;
        F.sell_lpr = P.lpr;
        F.lds_max = P.lds_max;
    }
    if (!P.swide.empty()) {  // mixed layout: the slices beyond 16 bits stream d_scols
        upload(c, F.d_swide, P.swide);
        F.sell_nnz_wide = P.nnz_wide;
    }
    HIPCHK(hipStreamSynchronize(c->stream));  // P's host buffers die at scope exit
    static_cast<FaDeviceState &>(*c) = std::move(F);
    if (c->lds_rows > 0) c->lds_halo = (int64_t)P.hidx.size();
}

}  // namespace cdfem

// ================================================================================================
extern "C" {

int cdfem_abi_version(void) { return CDFEM_ABI_VERSION; }

int cdfem_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int cdfem_create(int device, cdfem_ctx **out)
{
    if (!out) return CDFEM_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CDFEM_ERR_HIP;
    if (device < 0 || device >= n) return CDFEM_ERR_ARG;
    cdfem_ctx *c = new (std::nothrow) cdfem_ctx();
    if (!c) return CDFEM_ERR_HIP;
    c->device = device;
    const int rc = guarded(c, [&] {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->d_state.alloc(1);
        HIPCHK(hipMemset(c->d_state, 0, sizeof(KrylovState)));
        c->h_state.alloc(1);
        HIPCHK(hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device));
        return CDFEM_OK;
    });
    if (rc != CDFEM_OK) {
        cdfem_destroy(c);
        return CDFEM_ERR_HIP;
    }
    *out = c;
    return CDFEM_OK;
}

// the context's members release what they own: the buffers and events first, the streams last
void cdfem_destroy(cdfem_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    comm_destroy(c);
    delete c;
}

const char *cdfem_last_error(const cdfem_ctx *c) { return c ? c->err.c_str() : "null context"; }

int cdfem_synchronize(cdfem_ctx *c)
{
    return guarded(c, [&] {
        HIPCHK(hipStreamSynchronize(c->stream));
        return CDFEM_OK;
    });
}

int cdfem_alloc(cdfem_ctx *c, size_t bytes, void **dptr)
{
    return guarded(c, [&] {
        if (!dptr) throw ArgError("dptr is null");
        *dptr = raw_device_alloc(bytes ? bytes : 1);  // the caller's to release (cdfem_free)
        return CDFEM_OK;
    });
}

int cdfem_free(cdfem_ctx *c, void *dptr)
{
    return guarded(c, [&] {
        HIPCHK(hipFree(dptr));
        return CDFEM_OK;
    });
}

int cdfem_memcpy(cdfem_ctx *c, void *dst, int dw, const void *src, int sw, size_t bytes)
{
    return guarded(c, [&] {
        hipMemcpyKind k = dw == CDFEM_DEVICE ? (sw == CDFEM_DEVICE ? hipMemcpyDeviceToDevice
                                                                   : hipMemcpyHostToDevice)
                                             : (sw == CDFEM_DEVICE ? hipMemcpyDeviceToHost
                                                                   : hipMemcpyHostToHost);
        HIPCHK(hipMemcpyAsync(dst, src, bytes, k, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return CDFEM_OK;
    });
}

int cdfem_vec_axpby(cdfem_ctx *c, int64_t n, double a, const double *x, double b, double *y)
{
    return guarded(c, [&] {
        if (n < 0) throw ArgError("n < 0");
        if (n == 0) return CDFEM_OK;
        if (!x || !y) throw ArgError("null vector");
        HIPCHK(launch_axpby_n(c, n, a, x, b, y));
        HIPCHK(hipStreamSynchronize(c->stream));
        return CDFEM_OK;
    });
}

int cdfem_mesh_upload(cdfem_ctx *c, int dim, int order, int ne, const double *elem_verts,
                      int64_t nldofs, const int32_t *elem_dofs, int n_ess, const int32_t *ess_dofs)
{
    return guarded(c, [&] {
        if (dim != 2 && dim != 3) throw ArgError("dim must be 2 or 3");
        if (order < 1 || order > kMaxD1 - 1) throw ArgError("order out of range");
        if (ne <= 0 || nldofs <= 0 || !elem_verts || !elem_dofs) throw ArgError("empty mesh");
        if (nldofs >= (int64_t)1 << 31) throw ArgError("nldofs exceeds int32 indexing");
        if (n_ess < 0 || (n_ess > 0 && !ess_dofs)) throw ArgError("bad essential list");
        HIPCHK(hipSetDevice(c->device));
        free_mesh(c);
        c->dim = dim;
        c->p = order;
        c->d1 = order + 1;
        c->nd = dim == 3 ? c->d1 * c->d1 * c->d1 : c->d1 * c->d1;
        c->nv = 1 << dim;
        c->ne = ne;
        c->nl = nldofs;
        c->nblk = (ne + kLanes - 1) / kLanes;
        c->qlay = (dim == 3 && order >= 3) ? 1 : 0;
        if ((int64_t)c->nblk * kLanes * c->nd >= (int64_t)1 << 31) throw ArgError("E-vector exceeds int32 indexing");
        c->rule_op = make_rule(order, rule_points_1d(0, dim, order));
        c->rule_lf = make_rule(order, rule_points_1d(1, dim, order));
        c->rule_err = make_rule(order, rule_points_1d(2, dim, order));

        const int nd = c->nd;
        c->h_ess.assign(nldofs, 0);
        for (int i = 0; i < n_ess; ++i) {
            if (ess_dofs[i] < 0 || ess_dofs[i] >= nldofs) throw ArgError("essential dof out of range");
            c->h_ess[ess_dofs[i]] = 1;
        }
        c->h_dofs.assign(elem_dofs, elem_dofs + (size_t)ne * nd);
        for (int32_t g : c->h_dofs)
            if (g < 0 || g >= nldofs) throw ArgError("element dof out of range");
        std::vector<int32_t> ess_list;
        for (int64_t i = 0; i < nldofs; ++i)
            if (c->h_ess[i]) ess_list.push_back((int32_t)i);
        c->n_ess = (int)ess_list.size();

        c->mesh_affine = mesh_is_affine(dim, ne, elem_verts);
        upload(c, c->d_verts, elem_verts, (size_t)ne * c->nv * dim);
        upload(c, c->d_ess, c->h_ess);
        upload(c, c->d_ess_list, ess_list);
        c->d_dinv.alloc(nldofs);
        for (auto &w : c->d_w) w.alloc(nldofs);
        // element blocks of 64 in input order (identity permutation, padded)
        std::vector<int32_t> perm((size_t)c->nblk * kLanes, -1);
        for (int e = 0; e < ne; ++e) perm[e] = e;
        build_layout(c, perm);
        c->mesh_ready = true;
        return CDFEM_OK;
    });
}

int cdfem_mesh_set_structured(cdfem_ctx *c, int nx, int ny, int nz)
{
    return guarded(c, [&] {
        if (c->mesh_ready && c->geom != 0) throw ArgError("structured bricks need a hexahedral mesh");
        require_mesh(c);
        if (c->dim != 3) throw UnsupportedError("structured fast path is 3D only");
        if (nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny * nz != c->ne)
            throw ArgError("nx*ny*nz must equal the number of elements");
        const int p = c->p, d1 = c->d1, nd = c->nd;
        const int64_t Lx = (int64_t)p * nx + 1, Ly = (int64_t)p * ny + 1, Lz = (int64_t)p * nz + 1;
        if (Lx * Ly * Lz != c->nl) throw ArgError("dof count does not match the structured lattice");
        // the element dof map must be the lexicographic lattice numbering (cdfem_box_mesh)
        for (int e = 0; e < c->ne; ++e) {
            const int ix = e % nx, iy = (e / nx) % ny, iz = e / (nx * ny);
            for (int l = 0; l < nd; ++l) {
                const int dx = l % d1, dy = (l / d1) % d1, dz = l / (d1 * d1);
                const int64_t g = (p * ix + dx) + Lx * ((p * iy + dy) + Ly * (int64_t)(p * iz + dz));
                if (c->h_dofs[(size_t)e * nd + l] != g)
                    throw ArgError("element dof map is not the lexicographic structured numbering");
            }
        }
        c->sx = nx; c->sy = ny; c->sz = nz;
        c->Lx = Lx; c->Ly = Ly; c->Lz = Lz;
        if (c->qlay == 1) {
            // high order: lattice gather in the apply, pencil E-vector layout, lattice E->L
            // (k_e2l_box); element-major qdata and map are kept
            c->structured = true;
            c->epencil = c->nl < ((int64_t)1 << 32);
            c->hb_ez = c->ho_block_z;
            c->hb_nbx = (nx + kHoBrickEdge - 1) / kHoBrickEdge;
            c->hb_nby = (ny + kHoBrickEdge - 1) / kHoBrickEdge;
            c->hb_nbz = (nz + c->hb_ez - 1) / c->hb_ez;
            c->hb_nblk = c->hb_nbx * c->hb_nby * c->hb_nbz;
            upload_brick_ess(c, kHoBrickEdge, c->hb_ez, c->hb_nbx, c->hb_nby, c->hb_nbz);
            c->d_face.reset();  // the high-order brick CG's patch buffer: allocated by its first solve
            return CDFEM_OK;
        }
        c->nbx = (nx + kBrick - 1) / kBrick;
        c->nby = (ny + kBrick - 1) / kBrick;
        c->nbz = (nz + kBrick - 1) / kBrick;
        c->nblk = c->nbx * c->nby * c->nbz;
        upload_brick_ess(c, kBrick, kBrick, c->nbx, c->nby, c->nbz);
        // brick permutation: block = brick (lexicographic), lane = ex + 4 (ey + 4 ez)
        std::vector<int32_t> perm((size_t)c->nblk * kLanes, -1);
        for (int b = 0; b < c->nblk; ++b) {
            const int bx = b % c->nbx, by = (b / c->nbx) % c->nby, bz = b / (c->nbx * c->nby);
            for (int t = 0; t < kLanes; ++t) {
                const int ix = kBrick * bx + (t & 3), iy = kBrick * by + ((t >> 2) & 3),
                          iz = kBrick * bz + (t >> 4);
                if (ix < nx && iy < ny && iz < nz) perm[(size_t)b * kLanes + t] = ix + nx * (iy + ny * iz);
            }
        }
        build_layout(c, perm);
        const int S = kBrick * p + 1;
        c->nface = 2 * S * S + (S - 2) * (4 * S - 4);
        // per brick: the Mult's face partials (nface) or the CG apply's whole patch output (S^3)
        c->d_face.alloc((size_t)c->nblk * std::max(c->nface, S * S * S));
        c->d_qd.reset();
        c->structured = true;
        c->pa_ready = false;
        c->dinv_ready = false;
        return CDFEM_OK;
    });
}

int cdfem_set_slab(cdfem_ctx *c, int zlo_shared, int zhi_shared)
{
    return guarded(c, [&] {
        if (!c->structured) throw StateError("cdfem_mesh_set_structured must precede cdfem_set_slab");
        if (c->dim != 3) throw UnsupportedError("multi-rank slabs are 3D z-slabs");
        if ((zlo_shared || zhi_shared) && !c->comm) throw StateError("attach a communicator first");
        if (c->part_mode == 2) throw StateError("a general partition (cdfem_set_shared) is already declared");
        c->zlo_shared = zlo_shared != 0;
        c->zhi_shared = zhi_shared != 0;
        const int64_t n = c->Lx * c->Ly;
        c->part_mode = 1;
        c->slab_nl_max = c->nl;
        c->slab_nb_max = brick_count(c);
        if (multi_rank(c)) {  // (collective: every rank declares its slab) each rank's counts in its own slots
            const int R = c->nranks;
            std::vector<double> h((size_t)2 * R, 0.0);
            h[2 * c->rank] = (double)c->nl;
            h[2 * c->rank + 1] = (double)brick_count(c);
            DevBuf<double> d;
            upload(c, d, h);
            comm_allreduce(c, d, 2 * R);
            HIPCHK(hipMemcpyAsync(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            for (int k = 0; k < R; ++k) {
                c->slab_nl_max = std::max<int64_t>(c->slab_nl_max, (int64_t)h[2 * k]);
                c->slab_nb_max = std::max<int64_t>(c->slab_nb_max, (int64_t)h[2 * k + 1]);
            }
        }
        c->skip_lo = c->zlo_shared ? n : 0;  // the lower plane is owned by the rank below
        for (auto &b : c->d_if) {
            b.alloc(n);
            HIPCHK(hipMemsetAsync(b, 0, n * 8, c->stream));
        }
        c->dinv_ready = false;
        return CDFEM_OK;
    });
}

int cdfem_set_shared(cdfem_ctx *c, int n_nbr, const int32_t *nbr_ranks, const int64_t *nbr_off,
                     const int32_t *nbr_idx)
{
    return guarded(c, [&] {
        require_mesh(c);
        if (!c->comm) throw StateError("attach a communicator first");
        if (c->part_mode == 1) throw StateError("a slab partition (cdfem_set_slab) is already declared");
        if (n_nbr < 0 || (n_nbr > 0 && (!nbr_ranks || !nbr_off || !nbr_idx))) throw ArgError("bad neighbour lists");
        std::vector<int32_t> ranks(nbr_ranks, nbr_ranks + n_nbr);
        std::vector<int64_t> off(nbr_off, nbr_off + n_nbr + 1);
        if (n_nbr == 0) off.assign(1, 0);
        if (off[0] != 0) throw ArgError("nbr_off[0] must be 0");
        for (int k = 0; k < n_nbr; ++k) {
            if (ranks[k] < 0 || ranks[k] >= c->nranks || ranks[k] == c->rank) throw ArgError("bad neighbour rank");
            if (k > 0 && ranks[k] <= ranks[k - 1]) throw ArgError("neighbour ranks must be strictly ascending");
            if (off[k + 1] <= off[k]) throw ArgError("every neighbour shares at least one dof");
        }
        const int64_t ntot = off[n_nbr];
        if (ntot >= ((int64_t)1 << 31)) throw ArgError("too many shared entries");
        std::vector<int32_t> idx(nbr_idx, nbr_idx + ntot);
        // holders of every shared dof (ascending rank, this rank included) and the owner
        std::vector<int32_t> first_rank(c->nl, INT32_MAX);
        std::vector<std::vector<std::pair<int32_t, int32_t>>> contrib;  // per distinct dof: (rank, src)
        std::vector<int32_t> slot(c->nl, -1), dofs;
        for (int k = 0; k < n_nbr; ++k) {
            std::vector<uint8_t> seen;
            for (int64_t j = off[k]; j < off[k + 1]; ++j) {
                const int32_t d = idx[j];
                if (d < 0 || d >= c->nl) throw ArgError("shared dof out of range");
                if (slot[d] < 0) {
                    slot[d] = (int32_t)dofs.size();
                    dofs.push_back(d);
                    contrib.push_back({{c->rank, -1}});
                }
                auto &cl = contrib[slot[d]];
                for (auto &pr : cl)
                    if (pr.first == ranks[k]) throw ArgError("a dof appears twice in one neighbour list");
                cl.push_back({ranks[k], (int32_t)j});
                first_rank[d] = std::min(first_rank[d], ranks[k]);
            }
        }
        // ownership: a dof held by a lower rank is not owned here; those dofs must be the prefix
        int64_t n_not_owned = 0;
        for (int32_t d : dofs)
            if (first_rank[d] < c->rank) ++n_not_owned;
        for (int32_t d : dofs)
            if ((first_rank[d] < c->rank) != (d < n_not_owned))
                throw ArgError("local numbering must list the dofs owned by lower ranks first (owned true dofs = suffix)");
        std::vector<int32_t> soff(1, 0), src, owner;
        for (size_t i = 0; i < dofs.size(); ++i) {
            auto cl = contrib[i];
            std::sort(cl.begin(), cl.end());
            for (auto &pr : cl) src.push_back(pr.second);
            soff.push_back((int32_t)src.size());
            owner.push_back(cl.front().first == c->rank ? -1 : cl.front().second);
        }
        partition_free(c);
        c->nbr_rank = ranks;
        c->nbr_off = off;
        c->h_sh_idx = idx;
        c->n_shd = (int32_t)dofs.size();
        upload(c, c->d_sh_idx, idx);
        c->d_sh_send.alloc(ntot);
        c->d_sh_recv.alloc(ntot);
        upload(c, c->d_shd, dofs);
        upload(c, c->d_shd_off, soff);
        upload(c, c->d_shd_src, src);
        upload(c, c->d_shd_owner, owner);
        HIPCHK(hipStreamSynchronize(c->stream));
        c->part_mode = 2;
        c->skip_lo = n_not_owned;
        c->dinv_ready = false;
        return CDFEM_OK;
    });
}

// every shared entry's global id against the neighbour's entry at the same position: the shared
// sums pair slot j of a neighbour list with local dof idx[j] on both sides, so the lists must agree
// entry for entry (ascending global id); a mismatch fails on both ranks of the pair
int cdfem_check_shared(cdfem_ctx *c, const int64_t *l2g)
{
    return guarded(c, [&] {
        require_mesh(c);
        if (c->part_mode != 2) throw StateError("declare the partition first (cdfem_set_shared)");
        if (!l2g) throw ArgError("l2g is null");
        const int nn = (int)c->nbr_rank.size();
        const int64_t ntot = nn ? c->nbr_off[nn] : 0;
        if (nn == 0) return CDFEM_OK;
        // 1. list lengths first: mismatched send / recv counts would hang RCCL or misread
        //    the host buffers, so both ranks of a pair compare them before any id moves
        std::vector<int64_t> off1(nn + 1);
        std::vector<double> cs(nn), cr(nn);
        for (int k = 0; k <= nn; ++k) off1[k] = k;
        for (int k = 0; k < nn; ++k) cs[k] = (double)(c->nbr_off[k + 1] - c->nbr_off[k]);
        // (the counts travel in the send / recv buffers of the shared sums when they hold nn slots,
        //  else in scratch freed on every exit path, exceptions from the exchange included)
        DevBuf<double> sa, sb;
        double *d_a = c->d_sh_send, *d_b = c->d_sh_recv;
        if (ntot < nn) {
            sa.alloc(nn);
            sb.alloc(nn);
            d_a = sa;
            d_b = sb;
        }
        HIPCHK(hipMemcpyAsync(d_a, cs.data(), nn * 8, hipMemcpyHostToDevice, c->stream));
        comm_exchange_nbr_buf(c, off1, d_a, d_b, c->stream);
        HIPCHK(hipMemcpyAsync(cr.data(), d_b, nn * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < nn; ++k)
            if (cr[k] != cs[k])
                throw ArgError("shared-dof list with rank " + std::to_string(c->nbr_rank[k]) + " has " +
                               std::to_string((int64_t)cs[k]) + " entries here, " + std::to_string((int64_t)cr[k]) +
                               " there");
        // 2. the ids; an out-of-range id is reported after the exchange, so every rank stays in step
        std::vector<double> send((size_t)ntot), recv((size_t)ntot);
        int64_t bad = -1;
        for (int64_t j = 0; j < ntot; ++j) {
            const int64_t g = l2g[c->h_sh_idx[j]];
            const bool ok = g >= 0 && g < ((int64_t)1 << 53);
            if (!ok && bad < 0) bad = j;
            send[j] = ok ? (double)g : -1.0;  // exact below 2^53
        }
        HIPCHK(hipMemcpyAsync(c->d_sh_send, send.data(), ntot * 8, hipMemcpyHostToDevice, c->stream));
        comm_exchange_nbr_buf(c, c->nbr_off, c->d_sh_send, c->d_sh_recv, c->stream);
        HIPCHK(hipMemcpyAsync(recv.data(), c->d_sh_recv, ntot * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (bad >= 0)
            throw ArgError("global dof id out of range: " + std::to_string(l2g[c->h_sh_idx[bad]]) +
                           " (local dof " + std::to_string(c->h_sh_idx[bad]) + ")");
        for (int k = 0; k < nn; ++k)
            for (int64_t j = c->nbr_off[k]; j < c->nbr_off[k + 1]; ++j)
                if (recv[j] != send[j])
                    throw ArgError("shared-dof list with rank " + std::to_string(c->nbr_rank[k]) + " differs at entry " +
                                   std::to_string(j - c->nbr_off[k]) + ": global id " +
                                   std::to_string((int64_t)send[j]) + " here, " + std::to_string((int64_t)recv[j]) +
                                   " there (both sides must list the shared dofs in ascending global id)");
        return CDFEM_OK;
    });
}

int cdfem_true_size(cdfem_ctx *c, int64_t *ntrue, int64_t *first_owned)
{
    return guarded(c, [&] {
        require_mesh(c);
        if (ntrue) *ntrue = c->nl - c->skip_lo;
        if (first_owned) *first_owned = c->skip_lo;
        return CDFEM_OK;
    });
}

int cdfem_prolongate(cdfem_ctx *c, const double *X, double *x, int where)
{
    return guarded(c, [&] {
        require_mesh(c);
        require_partition(c);
        if (!X || !x) throw ArgError("null vector");
        const int64_t nt = c->nl - c->skip_lo;
        double *dx = where == CDFEM_DEVICE ? x : c->d_w[1];
        HIPCHK(hipMemsetAsync(dx, 0, c->skip_lo * 8, c->stream));
        HIPCHK(hipMemcpyAsync(dx + c->skip_lo, X, nt * 8, where == CDFEM_DEVICE ? hipMemcpyDeviceToDevice
                                                                                 : hipMemcpyHostToDevice, c->stream));
        interface_copy_owner(c, dx);
        dev_out(c, x, where, dx, c->nl);
        HIPCHK(hipStreamSynchronize(c->stream));
        return CDFEM_OK;
    });
}

// simplex meshes: points of a rule (and its reference coordinates); the operator's integrators have
// rules of their own (CDFEM_RULE_DIFFUSION / CONVECTION / MASS), so CDFEM_RULE_OPERATOR is refused
static int simplex_rule_pts(const cdfem_ctx *c, int rule, const std::vector<double> **sxi)
{
    const std::vector<double> *x = nullptr;
    int nq = 0;
    switch (rule) {
    case CDFEM_RULE_DIFFUSION: x = &c->h_sxi_d; nq = c->nq_sd; break;
    case CDFEM_RULE_CONVECTION:
    case CDFEM_RULE_MASS: x = &c->h_sxi_cm; nq = c->nq_scm; break;
    case CDFEM_RULE_LINEARFORM: x = &c->h_sxi_lf; nq = c->nq_lf; break;
    case CDFEM_RULE_NONLINEAR:
        if (!c->heat.ready) throw StateError("CDFEM_RULE_NONLINEAR: cdfem_nl_setup has not been called");
        x = &c->heat.h_sxi;
        nq = c->heat.nq;
        break;
    case CDFEM_RULE_OPERATOR:
        throw UnsupportedError("simplex meshes: each integrator has its own rule (CDFEM_RULE_DIFFUSION, "
                               "CDFEM_RULE_CONVECTION, CDFEM_RULE_MASS)");
    default: throw UnsupportedError("simplex meshes: no such rule (the L2-error rule is host-side)");
    }
    if (sxi) *sxi = x;
    return nq;
}

// quads / hexes: the 1D tables of a rule (CDFEM_RULE_NONLINEAR: after cdfem_nl_pa_setup)
static const Rule1D &tensor_rule(const cdfem_ctx *c, int rule)
{
    if (rule == CDFEM_RULE_NONLINEAR) {
        if (!c->heat.ready || !c->heat.tensor)
            throw StateError("CDFEM_RULE_NONLINEAR: neither cdfem_nl_pa_setup nor cdfem_nl_fa_setup has been called");
        return c->heat.rule;
    }
    return rule == CDFEM_RULE_LINEARFORM ? c->rule_lf : rule == CDFEM_RULE_ERROR ? c->rule_err : c->rule_op;
}

int cdfem_rule_size(cdfem_ctx *c, int rule, int *nq)
{
    return guarded(c, [&] {
        require_mesh(c);
        if (!nq) throw ArgError("nq is null");
        if (c->geom != 0) {
            *nq = simplex_rule_pts(c, rule, nullptr);
            return CDFEM_OK;
        }
        const Rule1D &r = tensor_rule(c, rule);
        *nq = nq_of(c, r);
        return CDFEM_OK;
    });
}

int cdfem_quadrature_points(cdfem_ctx *c, int rule, double *xyz, int where)
{
    return guarded(c, [&] {
        require_mesh(c);
        if (!xyz) throw ArgError("xyz is null");
        if (c->geom != 0) {  // affine simplices: x = v0 + J xi, evaluated on the host
            const std::vector<double> *psxi = nullptr;
            const int nq = simplex_rule_pts(c, rule, &psxi);
            const std::vector<double> &sxi = *psxi;
            const int dim = c->dim, nv = dim + 1;
            std::vector<double> out((size_t)c->ne * nq * dim);
            for (int e = 0; e < c->ne; ++e) {
                const double *V = &c->h_verts[(size_t)e * nv * dim];
                for (int q = 0; q < nq; ++q)
                    for (int k = 0; k < dim; ++k) {
                        double x = V[k];
                        for (int m = 0; m < dim; ++m) x += (V[(m + 1) * dim + k] - V[k]) * sxi[(size_t)q * dim + m];
                        out[((size_t)e * nq + q) * dim + k] = x;
                    }
            }
            if (where == CDFEM_DEVICE) {
                HIPCHK(hipMemcpyAsync(xyz, out.data(), out.size() * 8, hipMemcpyHostToDevice, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
            } else {
                std::copy(out.begin(), out.end(), xyz);
            }
            return CDFEM_OK;
        }
        const Rule1D &r = tensor_rule(c, rule);
        const size_t n = (size_t)c->ne * nq_of(c, r) * c->dim;
        DevBuf<double> tmp;
        if (where != CDFEM_DEVICE) tmp.alloc(n);
        double *d = where == CDFEM_DEVICE ? xyz : tmp.get();
        HIPCHK(launch_quad_points(c, r, d));
        if (where != CDFEM_DEVICE) {
            HIPCHK(hipMemcpyAsync(xyz, d, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        return CDFEM_OK;
    });
}

// device copy of an optional host coefficient array (null without one)
static DevBuf<double> upload_opt(cdfem_ctx *c, const double *h, size_t n)
{
    DevBuf<double> d;
    if (h) upload(c, d, h, n);
    return d;
}

static void check_form(const cdfem_ctx *c, const cdfem_form_coeffs *f)
{
    if (!f) throw ArgError("null form");
    if (f->kinds == 0 || f->kinds > 7) throw ArgError("kinds must be a non-empty DIFFUSION|CONVECTION|MASS mask");
    if ((f->kinds & CDFEM_CONVECTION) && !f->conv && !f->conv_q) throw ArgError("convection needs a velocity");
    (void)c;
}

static int pa_setup_form(cdfem_ctx *c, const cdfem_form_coeffs *f)
{
    return guarded(c, [&] {
        require_mesh(c);
        check_form(c, f);
        if (c->geom != 0) throw UnsupportedError("simplex meshes use full assembly: cdfem_fa_setup");
        if (!apply_supported(c->dim, c->p))
            throw UnsupportedError("no PA apply kernel built for dim=" + std::to_string(c->dim) +
                                   " order=" + std::to_string(c->p));
        const unsigned kinds = f->kinds;
        c->heat.jac_mf = false;  // the linear operator is the current one again
        c->kinds = kinds;
        c->ncomp = ((kinds & CDFEM_DIFFUSION) ? c->dim * (c->dim + 1) / 2 : 0) +
                   ((kinds & CDFEM_CONVECTION) ? c->dim : 0) + ((kinds & CDFEM_MASS) ? 1 : 0);
        const int nq = nq_of(c, c->rule_op);
        c->d_qd.alloc(c->qlay == 1 ? (size_t)c->ne * c->rule_op.q1 * qd_ho_plane(c->ncomp, c->rule_op.q1)
                                   : (size_t)c->nblk * nq * c->ncomp * kLanes);
        const size_t neq = (size_t)c->ne * nq;
        c->d_qaff.reset();
        if (c->pa_affine && c->mesh_affine && !f->kappa_q && !f->kappa_mat_q && !f->conv_q && !f->mass_q)
            c->d_qaff.alloc((size_t)c->nblk * c->ncomp * kLanes);
        // pa_geom: a hex mesh the affine forms did not take, constant coefficients, the thread-per-element
        // applies on the operator rule: the element geometry next to the stream (which the diagonal, the
        // linear system and a later pa_geom 0 still read).  Any other case keeps the stream alone.
        c->d_geom.reset();
        if (c->pa_geom && c->d_qaff == nullptr && c->dim == 3 && c->qlay == 0 && (c->p == 1 || c->p == 2) &&
            c->rule_op.q1 == c->p + 2 && !f->kappa_q && !f->kappa_mat_q && !f->conv_q && !f->mass_q) {
            c->d_geom.alloc(GeomLayout::kHdr + (size_t)c->nblk * GeomLayout::kNC * kLanes);
            double hdr[GeomLayout::kHdr] = {};
            hdr[GeomLayout::hKappa] = f->kappa;
            for (int i = 0; i < 3; ++i) hdr[GeomLayout::hConv + i] = ((kinds & CDFEM_CONVECTION) && f->conv) ? f->alpha * f->conv[i] : 0.0;
            hdr[GeomLayout::hMass] = f->mass;
            for (int q = 0; q < c->rule_op.q1; ++q) hdr[GeomLayout::hPts + q] = c->rule_op.pts[q];
            HIPCHK(hipMemcpy(c->d_geom, hdr, sizeof(hdr), hipMemcpyHostToDevice));
            HIPCHK(launch_setup_geom(c));
        }
        // ho_geom: the same for the p = 3, 4 tile apply, element-major (whether the apply takes it also
        // depends on ho_mfma when it runs: ho_geom_on)
        c->d_hgeom.reset();
        if (c->ho_geom && c->d_qaff == nullptr && c->dim == 3 && c->qlay == 1 && (c->p == 3 || c->p == 4) &&
            c->rule_op.q1 == c->p + 2 && !f->kappa_q && !f->kappa_mat_q && !f->conv_q && !f->mass_q) {
            c->d_hgeom.alloc(GeomLayout::kHdr + (size_t)c->ne * HoGeomLayout::kNC);
            double hdr[GeomLayout::kHdr] = {};
            hdr[GeomLayout::hKappa] = f->kappa;
            for (int i = 0; i < 3; ++i) hdr[GeomLayout::hConv + i] = ((kinds & CDFEM_CONVECTION) && f->conv) ? f->alpha * f->conv[i] : 0.0;
            hdr[GeomLayout::hMass] = f->mass;
            for (int q = 0; q < c->rule_op.q1; ++q) hdr[GeomLayout::hPts + q] = c->rule_op.pts[q];
            HIPCHK(hipMemcpy(c->d_hgeom, hdr, sizeof(hdr), hipMemcpyHostToDevice));
            HIPCHK(launch_setup_hgeom(c));
        }
        const DevBuf<double> dk = upload_opt(c, f->kappa_q, neq), dkm = upload_opt(c, f->kappa_mat_q, neq * c->dim * (c->dim + 1) / 2);
        const DevBuf<double> dc = upload_opt(c, f->conv_q, neq * c->dim), dm = upload_opt(c, f->mass_q, neq);
        HIPCHK(launch_setup_qdata(c, dk, dkm, f->kappa, f->alpha, f->conv, dc, dm, f->mass));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(setup_uniform_elem(c));  // pa_uniform: the common element matrix of a uniform box
        c->pa_ready = true;
        c->fa_ready = false;  // an assembled operator of this mesh is dropped (its pattern stays for the next one)
        c->dinv_ready = false;
        ilu_free(c);
        HIPCHK(setup_ho_uniform_elem(c));  // ho_uniform: the same for the p = 3, 4 block CG (reads the flags above)
        return CDFEM_OK;
    });
}

static int fa_setup_form(cdfem_ctx *c, const cdfem_form_coeffs *f);

int cdfem_pa_setup_form(cdfem_ctx *c, const cdfem_form_coeffs *f) { return pa_setup_form(c, f); }
int cdfem_fa_setup_form(cdfem_ctx *c, const cdfem_form_coeffs *f) { return fa_setup_form(c, f); }

int cdfem_pa_setup(cdfem_ctx *c, unsigned kinds, double kappa, const double *kappa_q, double alpha,
                   const double *conv, const double *conv_q, double mass, const double *mass_q)
{
    const cdfem_form_coeffs f{kinds, kappa, kappa_q, nullptr, alpha, conv, conv_q, mass, mass_q};
    return pa_setup_form(c, &f);
}

int cdfem_fa_setup(cdfem_ctx *c, unsigned kinds, double kappa, const double *kappa_q, double alpha,
                   const double *conv, const double *conv_q, double mass, const double *mass_q)
{
    const cdfem_form_coeffs f{kinds, kappa, kappa_q, nullptr, alpha, conv, conv_q, mass, mass_q};
    return fa_setup_form(c, &f);
}

int cdfem_mesh_upload_simplex(cdfem_ctx *c, int dim, int order, int ne, const double *elem_verts,
                              int64_t nldofs, const int32_t *elem_dofs, int n_ess, const int32_t *ess_dofs)
{
    return guarded(c, [&] {
        if (dim != 2 && dim != 3) throw ArgError("dim must be 2 or 3");
        if (order < 1 || order > (dim == 2 ? 3 : 2)) throw ArgError("simplex order: 1-3 (triangles), 1-2 (tets)");
        if (ne <= 0 || nldofs <= 0 || !elem_verts || !elem_dofs) throw ArgError("empty mesh");
        if (nldofs >= (int64_t)1 << 31) throw ArgError("nldofs exceeds int32 indexing");
        if (n_ess < 0 || (n_ess > 0 && !ess_dofs)) throw ArgError("bad essential list");
        HIPCHK(hipSetDevice(c->device));
        free_mesh(c);
        c->geom = 1;
        c->dim = dim;
        c->p = order;
        c->d1 = order + 1;
        c->nd = simplex_ndofs(dim, order);
        c->nv = dim + 1;
        c->ne = ne;
        c->nl = nldofs;
        c->nblk = (ne + kLanes - 1) / kLanes;
        const int nd = c->nd;
        c->h_ess.assign(nldofs, 0);
        for (int i = 0; i < n_ess; ++i) {
            if (ess_dofs[i] < 0 || ess_dofs[i] >= nldofs) throw ArgError("essential dof out of range");
            c->h_ess[ess_dofs[i]] = 1;
        }
        c->h_dofs.assign(elem_dofs, elem_dofs + (size_t)ne * nd);
        for (int32_t g : c->h_dofs)
            if (g < 0 || g >= nldofs) throw ArgError("element dof out of range");
        c->h_verts.assign(elem_verts, elem_verts + (size_t)ne * c->nv * dim);
        std::vector<int32_t> ess_list;
        for (int64_t i = 0; i < nldofs; ++i)
            if (c->h_ess[i]) ess_list.push_back((int32_t)i);
        c->n_ess = (int)ess_list.size();
        // the integrators' rules (MFEM's GetRule on affine simplices, tabulated rules): diffusion of
        // order 2p - 2, convection and mass of order 2p; basis tables of both, diffusion first
        std::vector<double> wd, wcm, tab;
        c->nq_sd = simplex_rule_for_order(dim, std::max(2 * order - 2, 0), c->h_sxi_d, wd);
        c->nq_scm = simplex_rule_for_order(dim, 2 * order, c->h_sxi_cm, wcm);
        for (int r = 0; r < 2; ++r) {
            const std::vector<double> &xi = r == 0 ? c->h_sxi_d : c->h_sxi_cm, &w = r == 0 ? wd : wcm;
            const int nq = r == 0 ? c->nq_sd : c->nq_scm;
            const size_t o = tab.size();
            tab.resize(o + (size_t)nq * nd * (dim + 1) + nq);
            for (int q = 0; q < nq; ++q) {
                double phi[10], dphi[30];
                simplex_basis(dim, order, &xi[(size_t)q * dim], phi, dphi);
                for (int i = 0; i < nd; ++i) {
                    tab[o + (size_t)q * nd + i] = phi[i];
                    for (int k = 0; k < dim; ++k)
                        tab[o + (size_t)nq * nd + ((size_t)q * nd + i) * dim + k] = dphi[i * dim + k];
                }
                tab[o + (size_t)nq * nd * (dim + 1) + q] = w[q];
            }
        }
        // linear-form rule: DomainLFIntegrator's default order 2p, MFEM's tabulated simplex rule
        std::vector<double> wl;
        c->nq_lf = simplex_rule_for_order(dim, 2 * order, c->h_sxi_lf, wl);
        std::vector<double> tab_lf((size_t)c->nq_lf * (nd + 1));
        for (int q = 0; q < c->nq_lf; ++q) {
            double phi[10], dphi[30];
            simplex_basis(dim, order, &c->h_sxi_lf[(size_t)q * dim], phi, dphi);
            for (int i = 0; i < nd; ++i) tab_lf[(size_t)q * nd + i] = phi[i];
            tab_lf[(size_t)c->nq_lf * nd + q] = wl[q];
        }
        // E->L transpose of the element-major E-vector (linear forms)
        std::vector<int32_t> cnt(nldofs + 1, 0), pos((size_t)ne * nd);
        for (int32_t g : c->h_dofs) cnt[g + 1]++;
        for (int64_t i = 0; i < nldofs; ++i) cnt[i + 1] += cnt[i];
        {
            std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
            for (int64_t k = 0; k < (int64_t)ne * nd; ++k) pos[fill[c->h_dofs[k]]++] = (int32_t)k;
        }
        upload(c, c->d_e2l_off, cnt);
        upload(c, c->d_e2l_pos, pos);
        c->d_Ye.alloc(pos.size());
        upload(c, c->d_stab_lf, tab_lf);
        upload(c, c->d_stab, tab);
        upload(c, c->d_verts, c->h_verts);
        upload(c, c->d_ess, c->h_ess);
        upload(c, c->d_ess_list, ess_list);
        c->d_dinv.alloc(nldofs);
        for (auto &v : c->d_w) v.alloc(nldofs);
        c->d_part.alloc((size_t)c->red_blocks + kSpmvMaxBlocks + 16384);
        HIPCHK(hipStreamSynchronize(c->stream));
        c->mesh_ready = true;
        return CDFEM_OK;
    });
}

// quads and hexes (inside guarded): the element matrices of k_tensor_elem on the OPERATOR rule, then the
// simplex pipeline.  The PA operator, the matrix-free Jacobian, the Jacobi scale and the ILU factors of the
// previous operator are dropped; the pattern of an earlier assembly on this mesh is reused.
static void fa_setup_tensor(cdfem_ctx *c, const cdfem_form_coeffs *f)
{
    if (!fa_tensor_supported(c->dim, c->p))
        throw UnsupportedError("full assembly on tensor meshes is built for quads p = 1..4 and hexes p = 1, 2 (dim=" +
                               std::to_string(c->dim) + " order=" + std::to_string(c->p) + ")");
    if (multi_rank(c)) throw UnsupportedError("full assembly on quad and hex meshes runs on one rank");
    fa_ensure_pattern(c);
    // per-point coefficients at the OPERATOR rule's points (cdfem_quadrature_points' order)
    const size_t neq = (size_t)c->ne * nq_of(c, c->rule_op);
    const DevBuf<double> dk = upload_opt(c, f->kappa_q, neq), dkm = upload_opt(c, f->kappa_mat_q, neq * c->dim * (c->dim + 1) / 2);
    const DevBuf<double> dc = upload_opt(c, f->conv_q, neq * c->dim), dm = upload_opt(c, f->mass_q, neq);
    c->kinds = f->kinds;
    HIPCHK(launch_tensor_elem(c, dk, dkm, f->kappa, f->alpha, f->conv, dc, dm, f->mass));
    HIPCHK(launch_fa_assemble(c));
    HIPCHK(launch_sell_fill(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->fa_ready = true;
    c->pa_ready = false;
    c->heat.jac_mf = false;
    c->dinv_ready = false;
    ilu_free(c);  // factors belong to the previous operator
}

static int fa_setup_form(cdfem_ctx *c, const cdfem_form_coeffs *f)
{
    return guarded(c, [&] {
        require_mesh(c);
        check_form(c, f);
        const unsigned kinds = f->kinds;
        if (c->geom != 1) {
            fa_setup_tensor(c, f);
            return CDFEM_OK;
        }
        fa_ensure_pattern(c);
        // per-point coefficients at the rule of their integrator
        const size_t nqd = (size_t)c->ne * c->nq_sd, nqc = (size_t)c->ne * c->nq_scm;
        const DevBuf<double> dk = upload_opt(c, f->kappa_q, nqd), dkm = upload_opt(c, f->kappa_mat_q, nqd * c->dim * (c->dim + 1) / 2);
        const DevBuf<double> dc = upload_opt(c, f->conv_q, nqc * c->dim), dm = upload_opt(c, f->mass_q, nqc);
        c->kinds = kinds;
        HIPCHK(launch_simplex_elem(c, dk, dkm, f->kappa, f->alpha, f->conv, dc, dm, f->mass));
        HIPCHK(launch_fa_assemble(c));
        HIPCHK(launch_sell_fill(c));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->fa_ready = true;
        c->pa_ready = false;
        c->dinv_ready = false;
        ilu_free(c);  // factors belong to the previous operator
        return CDFEM_OK;
    });
}

int cdfem_fa_csr(cdfem_ctx *c, int constrained, int64_t *nnz, int32_t *rowptr, int32_t *cols, double *vals)
{
    return guarded(c, [&] {
        if (!c->fa_ready) throw StateError("cdfem_fa_setup has not been called");
        if (!nnz) throw ArgError("nnz is null");
        *nnz = c->nnz;
        if (rowptr) HIPCHK(hipMemcpy(rowptr, c->d_rowptr, (c->nl + 1) * 4, hipMemcpyDeviceToHost));
        if (cols) HIPCHK(hipMemcpy(cols, c->d_cols, c->nnz * 4, hipMemcpyDeviceToHost));
        if (vals)
            HIPCHK(hipMemcpy(vals, constrained ? c->d_vals_c : c->d_vals, c->nnz * 8, hipMemcpyDeviceToHost));
        return CDFEM_OK;
    });
}

int cdfem_pa_mult(cdfem_ctx *c, const double *x, double *y, int constrained, int where)
{
    return guarded(c, [&] {
        require_pa(c);
        if (constrained != 2) require_partition(c);
        if (!x || !y) throw ArgError("null vector");
        if (constrained < 0 || constrained > 2) throw ArgError("constrained must be 0, 1 or 2 (local)");
        const double *dx = dev_in(c, x, where, c->d_w[0], c->nl);
        double *dy = where == CDFEM_DEVICE ? y : c->d_w[1];
        if (constrained == 2) op_apply(c, dx, dy, false);  // rank-local partial sums (no exchange)
        else op_apply_global(c, dx, dy, constrained != 0);  // shared dofs: neighbours' partial sums added
        dev_out(c, y, where, dy, c->nl);
        prof_collect(c);
        return CDFEM_OK;
    });
}

int cdfem_pa_diagonal(cdfem_ctx *c, double *diag, int where)
{
    return guarded(c, [&] {
        require_pa(c);
        if (!diag) throw ArgError("null vector");
        double *dd = where == CDFEM_DEVICE ? diag : c->d_w[1];
        if (c->fa_ready) {
            HIPCHK(launch_csr_diag(c, dd));
        } else {
            timed(c, CDFEM_K_DIAGONAL, [&] { HIPCHK(launch_diag_elem(c, c->d_Ye)); });
            HIPCHK(launch_e2l(c, c->d_Ye, nullptr, dd, false, 0));
        }
        dev_out(c, diag, where, dd, c->nl);
        prof_collect(c);
        return CDFEM_OK;
    });
}

int cdfem_lf_assemble(cdfem_ctx *c, const double *f_q, double *b, int where)
{
    return guarded(c, [&] {
        require_mesh(c);
        if (!f_q || !b) throw ArgError("null vector");
        const size_t n = (size_t)c->ne * (c->geom != 0 ? c->nq_lf : nq_of(c, c->rule_lf));
        if (c->d_lfq.size() < n) c->d_lfq.alloc(n);  // kept: a time loop assembles a linear form every step
        double *dfq = c->d_lfq;
        HIPCHK(hipMemcpyAsync(dfq, f_q, n * 8, where == CDFEM_DEVICE ? hipMemcpyDeviceToDevice
                                                                     : hipMemcpyHostToDevice, c->stream));
        double *db = where == CDFEM_DEVICE ? b : c->d_w[1];
        if (c->geom != 0) HIPCHK(launch_simplex_lf(c, dfq, c->d_Ye));
        else HIPCHK(launch_lf_elem(c, dfq, c->d_Ye));
        HIPCHK(launch_e2l(c, c->d_Ye, nullptr, db, false, 0));
        dev_out(c, b, where, db, c->nl);
        HIPCHK(hipStreamSynchronize(c->stream));
        return CDFEM_OK;
    });
}

int cdfem_form_linear_system(cdfem_ctx *c, const double *x, const double *b, double *X, double *B,
                             int where)
{
    return guarded(c, [&] {
        require_pa(c);
        require_partition(c);
        if (!x || !b || !X || !B) throw ArgError("null vector");
        const double *dx = dev_in(c, x, where, c->d_w[0], c->nl);
        const double *db = dev_in(c, b, where, c->d_w[1], c->nl);
        double *xe = c->d_w[2], *z = c->d_w[3];
        double *dB = where == CDFEM_DEVICE ? B : c->d_w[4];
        HIPCHK(launch_mask_ess(c, dx, xe));                 // x_e: essential part of x
        op_apply(c, xe, z, false);                          // z = A x_e
        if (dB != db) HIPCHK(hipMemcpyAsync(dB, db, c->nl * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(launch_axpby(c, -1.0, z, 1.0, dB));          // B = b - A x_e
        interface_sum(c, dB);                               // P^T on the shared planes
        HIPCHK(launch_set_ess(c, dB, dx));                  // B[ess] = x[ess]
        dev_out(c, B, where, dB, c->nl);
        dev_out(c, X, where, dx, c->nl);
        HIPCHK(hipStreamSynchronize(c->stream));
        prof_collect(c);
        return CDFEM_OK;
    });
}

int cdfem_solve(cdfem_ctx *c, const cdfem_solver_params *p, const double *B, double *X, int where,
                cdfem_solver_result *res)
{
    return guarded(c, [&] {
        require_pa(c);
        require_partition(c);
        if (!p || !B || !X || !res) throw ArgError("null argument");
        *res = cdfem_solver_result{};
        check_solver_params(*p);
        c->last_method = p->method;
        const double *dB = dev_in(c, B, where, c->d_w[6], c->nl);
        double *dX = where == CDFEM_DEVICE ? X : c->d_w[1];
        solve_mesh_order(c, *p, dB, dX, *res);
        dev_out(c, X, where, dX, c->nl);
        HIPCHK(hipStreamSynchronize(c->stream));
        return res->converged ? CDFEM_OK : CDFEM_ERR_NOT_CONVERGED;
    });
}

int cdfem_stream_bench(cdfem_ctx *c, int mode, size_t bytes, int reps, double *gbps)
{
    return guarded(c, [&] {
        if (!gbps || reps < 1 || mode < 0 || mode > 17) throw ArgError("bad stream bench arguments");
        int64_t n = (int64_t)(bytes / 16) * 2;
        if (mode >= 3) n = n / 40960 * 40960;  // whole 320 KiB chunks
        DevBuf<double> a, b;
        a.alloc(n);
        b.alloc(n);
        HIPCHK(hipMemsetAsync(a, 0, n * 8, c->stream));
        HIPCHK(hipMemsetAsync(b, 0, n * 8, c->stream));
        HIPCHK(launch_stream(c, mode, a, b, n));  // warm-up
        Event e0, e1;
        e0.create(true);
        e1.create(true);
        HIPCHK(hipEventRecord(e0, c->stream));
        for (int i = 0; i < reps; ++i) HIPCHK(launch_stream(c, mode, a, b, n));
        HIPCHK(hipEventRecord(e1, c->stream));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        double moved = (mode == 2 ? 2.0 : 1.0) * 8.0 * (double)n * reps;
        if (mode == 14 || mode == 15) {  // workgroup chunks: whole groups of 4 / 2 chunks
            const int64_t nw = mode == 14 ? 4 : 2;
            moved = 8.0 * 40960.0 * (double)(n / 40960 / nw * nw) * reps;
        }
        if (mode >= 10 && mode <= 13) {  // skewed chunks: whole 320 KiB chunks at a stride of 320 KiB + skew
            const int64_t skew[4] = {32, 64, 128, 512};
            moved = 8.0 * 40960.0 * (double)(n / (40960 + skew[mode - 10])) * reps;
        }
        *gbps = moved / (ms * 1e-3) / 1e9;
        return CDFEM_OK;
    });
}

int cdfem_fp64_bench(cdfem_ctx *c, int mode, int reps, double *tflops)
{
    return guarded(c, [&] {
        if (!tflops || reps < 1 || mode < 0 || mode > 4) throw ArgError("bad fp64 bench arguments");
        DevBuf<double> out;
        out.alloc(1);
        double flops = 0.0;
        HIPCHK(launch_fp64_probe(c, mode, out, &flops));  // warm-up
        Event e0, e1;
        e0.create(true);
        e1.create(true);
        HIPCHK(hipEventRecord(e0, c->stream));
        for (int i = 0; i < reps; ++i) HIPCHK(launch_fp64_probe(c, mode, out, &flops));
        HIPCHK(hipEventRecord(e1, c->stream));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *tflops = flops * reps / (ms * 1e-3) / 1e12;
        return CDFEM_OK;
    });
}

int cdfem_set_option(cdfem_ctx *c, const char *key, int value)
{
    return guarded(c, [&] {
        const std::string refusal = set_option(*c, key, value);
        if (!refusal.empty()) throw ArgError(refusal);
        return CDFEM_OK;
    });
}

int cdfem_profile_enable(cdfem_ctx *c, int on)
{
    return guarded(c, [&] {
        c->profile = on != 0;
        return CDFEM_OK;
    });
}

int cdfem_profile_reset(cdfem_ctx *c)
{
    return guarded(c, [&] {
        for (auto &s : c->prof) {
            s.used = 0;
            s.total_ms = 0.0;
            s.count = 0;
            s.each.clear();
        }
        return CDFEM_OK;
    });
}

int cdfem_profile_read(cdfem_ctx *c, int k, double *total_ms, int64_t *count)
{
    return guarded(c, [&] {
        if (k < 0 || k >= CDFEM_K_COUNT) throw ArgError("bad kernel id");
        if (total_ms) *total_ms = c->prof[k].total_ms;
        if (count) *count = c->prof[k].count;
        return CDFEM_OK;
    });
}

int cdfem_profile_launches(cdfem_ctx *c, int k, double *ms, int64_t cap, int64_t *count)
{
    return guarded(c, [&] {
        if (k < 0 || k >= CDFEM_K_COUNT) throw ArgError("bad kernel id");
        const auto &e = c->prof[k].each;
        const int64_t n = (int64_t)e.size();
        if (count) *count = n;
        if (ms)
            for (int64_t i = 0; i < std::min(cap, n); ++i) ms[i] = e[i];
        return CDFEM_OK;
    });
}

// the cost model (model.hip)
int cdfem_kernel_name(cdfem_ctx *c, int k, char *buf, size_t n)
{
    return guarded(c, [&] {
        require_pa(c);
        if (!buf || n == 0) throw ArgError("buffer is null");
        kernel_name(c, k, buf, n);
        return CDFEM_OK;
    });
}

int cdfem_kernel_flops(cdfem_ctx *c, int k, double *flops)
{
    return guarded(c, [&] {
        require_pa(c);
        if (!flops) throw ArgError("flops is null");
        *flops = kernel_flops(c, k);
        return CDFEM_OK;
    });
}

int cdfem_kernel_bytes(cdfem_ctx *c, int k, double *bytes)
{
    return guarded(c, [&] {
        require_pa(c);
        if (!bytes) throw ArgError("bytes is null");
        *bytes = kernel_bytes(c, k);
        return CDFEM_OK;
    });
}

}  // extern "C"
