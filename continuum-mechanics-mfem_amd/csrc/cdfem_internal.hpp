// cdfem_internal.hpp — context layout and kernel-launch declarations shared by the HIP sources.
//
// Device data layout (HBM), chosen for the thread-per-element PA kernels:
//   elements are grouped in blocks of 64 (one wavefront, lane = element within the block);
//   elem map   : int32 [nblk][nd][64]      L-dof of local dof l of element 64*b+lane; essential
//                                           dofs stored as -(gid+1) so the constrained gather
//                                           reads 0 without a second array
//   qdata      : f64   [nblk][nq][nc][64]  per quadrature point: D (sym, dim(dim+1)/2), C (dim),
//                                           M (1), only the kinds present (nc = 7 for K+M, 10 all)
//   E-vector Y : f64   [nblk][nd][64]      element outputs before the E->L sum
//   E->L map   : CSR over L-dofs, entries = positions in Y, element order ascending (deterministic)
// Every wave reads 512 contiguous bytes per qdata component, so the dominant stream is fully
// coalesced; the x gather is served by L2/MALL (x is 17 MB at 64^3 p=2).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cdfem.h"
#include "ctx_state.hpp"
#include "dispatch.hpp"
#include "krylov_host.hpp"
#include "options.hpp"

namespace cdfem {

constexpr int kLanes = 64;        // elements per element-block (= wavefront width)
// (kMaxD1, kMaxQ1 and Rule1D, the 1D tables of one quadrature rule: ctx_state.hpp)

// Product implementation of the 1D rules (independent of the oracle): basis.cpp
void gll_nodes(int p, double *x);
void gauss_legendre(int n, double *x, double *w);
// simplices (basis.cpp)
int simplex_rule(int dim, int n, std::vector<double> &xi, std::vector<double> &w);
// MFEM's tabulated triangle (order <= 9) / tetrahedron (order <= 6) rules; 0 when not tabulated
int mfem_simplex_rule(int dim, int order, std::vector<double> &xi, std::vector<double> &w);
// the rule IntRules.Get(simplex, order) returns: MFEM's table, else collapsed Gauss of that order
int simplex_rule_for_order(int dim, int order, std::vector<double> &xi, std::vector<double> &w);
int simplex_ndofs(int dim, int p);
void simplex_basis(int dim, int p, const double *xi, double *phi, double *dphi);
// the same with the P3 tables formed in long double (1 ulp): for forms that interpolate a state from nodal values
void simplex_basis_x(int dim, int p, const double *xi, double *phi, double *dphi);
extern const int kSimplexEdge[6][2];
double p3_edge_t(int k);
// element partition helpers (partition.cpp, host only)
void partition_rcb(int dim, int ne, int nv, const double *elem_verts, int nranks, int32_t *part);
void p3_tri_nodes(double (*X)[2]);
extern const int kTriEdge[3][2];
Rule1D make_rule(int p, int q1);
// MFEM default rule sizes on multilinear tensor elements (which: 0 operator, 1 LF, 2 L2 error)
int rule_points_1d(int which, int dim, int p);

// High-order qdata layout (cdfem_ctx::qlay = 1, 3D p >= 3, ho_kernels.hip): per element and
// quadrature plane qz one block of nc * Q1^2 doubles (padded to an even count so every block is
// 16-byte aligned), components paired as [pair][qxy][2] with an odd last component as [qxy].
__host__ __device__ constexpr int qd_ho_plane(int nc, int q1) { return (nc * q1 * q1 + 1) & ~1; }
__host__ __device__ inline size_t qd_ho_index(int64_t e, int c, int q, int nc, int q1)
{
    const int qq = q1 * q1, qz = q / qq, qxy = q - qz * qq;
    const size_t base = ((size_t)e * q1 + qz) * qd_ho_plane(nc, q1);
    return base + ((c < (nc & ~1)) ? ((size_t)(c >> 1) * qq + qxy) * 2 + (c & 1) : (size_t)(nc & ~1) * qq + qxy);
}

// Device-side Krylov state (one per context), updated only by kernels.
struct KrylovState {
    double nom, nom0, den, alpha, beta, betanom, r0;
    double red[4];  // rank-local reductions awaiting the all-reduce (0 den, 1 betanom, 2 nom)
    int iter, done, converged, final_iter, max_iter, first_den;
    int xflush;     // x-fold CG (cg_xfold): the last update's x += alpha d is still pending (stopped by
                    // the update logic, so no further apply folded it): k_cg_xflush applies it
};

// Device-side GMRES(m) state (gmres.hip).  The host polls the head: the pinned slots hold heads (post_head)
constexpr int kGmMaxRestart = 64;
struct GmresHead {
    int cycle_done, done, converged, its;
    double res;
    int j, kk;
};
struct GmresState : GmresHead {
    int max_it, m;
    double ttol, res0;
    double s[kGmMaxRestart + 1];   // basis scales: v_i = s_i * V_i
    double g[kGmMaxRestart + 1], cs[kGmMaxRestart], sn[kGmMaxRestart];
    double H[(kGmMaxRestart + 1) * kGmMaxRestart];  // row-major, leading dimension kGmMaxRestart
    double red[kGmMaxRestart + 1];  // multi-rank: rank-local sums awaiting the all-reduce
    double y[kGmMaxRestart];        // cycle end: the least-squares solution, scaled by s
};

// Device-side BiCGStab state (bicgstab.hip), its head polled as GMRES's is.
enum : int { kBcgsBreakRho = 1, kBcgsBreakD1 = 2, kBcgsBreakD2 = 3 };  // BcgsState::breakdown
constexpr int kBcgsSlots = 4;  // pinned poll slots of the iterations, + 1 for the start
struct BcgsHead {
    int done, converged, its, breakdown;
    double dp;
};
struct BcgsState : BcgsHead {
    int half, max_it;              // half: d2 == 0, the x update adds alpha p alone and the solve ends
    double ttol, res0, rho, alpha, omega, beta, ss;
    double red[4];                 // multi-rank: rank-local sums awaiting the all-reduce
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"  // (a state with a base is not standard-layout: base first)
static_assert(sizeof(GmresHead) == 32 && offsetof(GmresState, cycle_done) == 0 && offsetof(GmresState, max_it) == 32);
static_assert(sizeof(BcgsHead) == 24 && offsetof(BcgsState, done) == 0 && offsetof(BcgsState, half) == 24);
#pragma clang diagnostic pop

// A captured graph and its executable, destroyed with their owner
struct SweepGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    SweepGraph() = default;
    SweepGraph(const SweepGraph &) = delete;
    SweepGraph &operator=(const SweepGraph &) = delete;
    SweepGraph(SweepGraph &&o) noexcept : graph(std::exchange(o.graph, nullptr)), exec(std::exchange(o.exec, nullptr)) {}
    SweepGraph &operator=(SweepGraph &&o) noexcept
    {
        std::swap(graph, o.graph);  // (o, a temporary or a state on its way out, destroys what this held)
        std::swap(exec, o.exec);
        return *this;
    }
    ~SweepGraph()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

// ILU(0) preconditioner state (ilu_kernels.hip); ilu_free assigns a default one
struct IluState {
    bool ready = false;
    DevBuf<double> F;                    // factors in the pattern below (unit-lower L, U packed)
    DevBuf<int32_t> rows_l, rows_u;      // rows grouped by level
    std::vector<int32_t> ptr_l, ptr_u;   // level pointers (host)
    DevBuf<double> z;                    // output of one application
    // multi-rank (PETSc bjacobi, one ILU(0) block per rank): the factored matrix is the owned
    // diagonal block of the global eliminated matrix, on rows/columns [skip_lo, nl), in its own
    // pattern; the sweeps write the owned part of z and the owners' values are then copied to the
    // non-owned shared entries
    bool block = false;
    DevBuf<int32_t> b_rp, b_cols, b_diag;  // the block's own pattern (block only)
    const int32_t *rp = nullptr, *cols = nullptr, *diag = nullptr;  // the pattern factored: the block's, else the CSR's
    int64_t nnz = 0;
    SweepGraph sweeps;                   // the captured forward + backward sweeps
};

struct Comm;  // comm.hip

struct ProfileSlot {
    std::vector<Event> ev;  // pairs
    int used = 0;
    double total_ms = 0.0;
    int64_t count = 0;
    std::vector<float> each;  // per-launch ms since the last reset (cdfem_profile_launches)
};

// The context's streams, a base of ContextState so that they are destroyed after everything the context owns
struct Streams {
    Streams() = default;
    Streams(const Streams &) = delete;
    Streams &operator=(const Streams &) = delete;
    ~Streams()
    {
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;      // side stream of the overlapped exchange (created on first use)
};

// What lives as long as the context: the Krylov drivers' device state with its pinned slots and events, the
// profiling slots, the communicator; and the description of the current mesh, which every upload assigns
// before mesh_ready and everything reads behind require_mesh / require_pa.  Declared ahead of the bases
// that own the mesh's buffers, so destroyed after them.
struct ContextState : Streams {
    int device = 0;
    Event ov_ev[2];                     // fork / join of the side stream
    std::string err;
    int ncu = 0;                        // compute units of the device
    Comm *comm = nullptr;               // rank communicator (comm.hip), nullptr on one GPU
    int rank = 0, nranks = 1;

    // mesh / space
    int dim = 0, p = 0, d1 = 0, nd = 0, ne = 0, nblk = 0, nv = 0;
    int qlay = 0;                       // 0: element blocks of 64 (thread per element), 1: element-major
                                        //    map / E-vector / qdata (wave per element, 3D p >= 3)
    int64_t nl = 0;
    int n_ess = 0;
    std::vector<int32_t> h_dofs;        // host copy of the element dof map (ne*nd)
    std::vector<uint8_t> h_ess;         // host essential marker (nl)
    bool mesh_affine = false;           // every element a parallelepiped (checked at upload)
    Rule1D rule_op, rule_lf, rule_err;
    // simplex integrator rules (MFEM's GetRule on affine simplices): diffusion order 2p - 2,
    // convection and mass order 2p, each on MFEM's tabulated rule (simplex_rule_for_order)
    int nq_sd = 0, nq_scm = 0;          // points of the diffusion / convection + mass rules
    int nq_lf = 0;                      // simplex LINEARFORM rule (collapsed Gauss, n = p + 3)

    // structured box (cdfem_mesh_set_structured)
    int sx = 0, sy = 0, sz = 0;         // elements per axis of the local box
    int nbx = 0, nby = 0, nbz = 0;      // bricks per axis
    // 3D p = 3, 4 on a structured box: blocks of kHoBrickEdge^3 elements for the high-order brick CG
    // (brick_kernels.hip k_hobrick_cg; set_option "ho_brick")
    int hb_nbx = 0, hb_nby = 0, hb_nbz = 0;
    int hb_ez = 2;                      //   the block depth of the current structured box
    int64_t Lx = 0, Ly = 0, Lz = 0;     // dof lattice per axis
    int nface = 0;                      // F of d_face
    double *den_out = nullptr;          // k_brick_cg writes its den partials here instead of d_part (set by the solve)
    bool udiag_bitwise = false;         // d_udiag: every non-essential entry of d_dinv equals its class entry bitwise
    int hoelem_p = 0;                   // d_hoelem: the order and kinds it was formed for
    unsigned hoelem_kinds = 0;
    double h_ktab[4 * 5 * 5] = {};      // d_ktab's host copy (source of the async upload)
    int64_t lds_halo = 0;               // staged columns over all windows of the LDS layout
    bool perm_space = false;            // inside a solve that runs in the permuted order

    // the operator
    unsigned kinds = 0;
    int ncomp = 0;

    // Krylov drivers
    int red_blocks = 1024;
    DevBuf<KrylovState> d_state;
    PinBuf<KrylovState> h_state;
    DevBuf<GmresState> d_gmst;          // device GMRES state
    PinBuf<GmresHead> h_gmpoll;         // kGmMaxRestart + 1 poll slots
    Event gm_ev[2];
    DevBuf<BcgsState> d_bcst;           // device BiCGStab state
    PinBuf<BcgsHead> h_bcpoll;          // kBcgsSlots + 1 poll slots
    Event bc_ev[2];
    int last_method = -1;               // method of the last cdfem_solve (kernel_bytes / kernel_name of CDFEM_K_UPDATE)
    int bcgs_src = 0;                   // the last BiCGStab solve's operator source: 0 the Mult's output, else the patch side
    int bcgs_diag = 0;                  // the last BiCGStab solve read a Jacobi diagonal
    EptCache gm_ept_auto, bcgs_ept_auto;  // entries per thread of the GMRES / BiCGStab vector kernels (pick_ept)

    // profiling
    bool profile = false;
    ProfileSlot prof[CDFEM_K_COUNT];
    hipEvent_t ext_ev[2] = {};  // armed by prof_mark(begin): the next CDFEM_LAUNCH records these
                                // events at its own dispatch start / end (hipExtLaunchKernelGGL)
};

}  // namespace cdfem

// the set_option switches and their defaults (options.hpp), then the state grouped by lifetime: the
// context's, the uploaded mesh's and the declared partition's (ctx_state.hpp), and the ILU(0) factors of
// the current operator and partition (ilu_free; GMRES pc = ILU)
struct cdfem_ctx : cdfem::Options, cdfem::ContextState, cdfem::MeshState, cdfem::PartitionState {
    cdfem::IluState ilu;
};

// Launch on the context stream; when a profiling mark is armed (prof_mark), the kernel records the
// mark's event pair itself at dispatch start and completion (hipExtLaunchKernelGGL), so the timed
// interval is the kernel alone, without the ~5-10 us an event record adds ahead of a ~100 us
// kernel.  Used for the dominant (roofline) kernels.
#define CDFEM_LAUNCH(c, kernel, grid, block, shm, ...)                                                       \
    do {                                                                                                     \
        if ((c)->ext_ev[0]) {                                                                                \
            hipExtLaunchKernelGGL(kernel, grid, block, shm, (c)->stream, (c)->ext_ev[0], (c)->ext_ev[1], 0,   \
                                  __VA_ARGS__);                                                              \
            (c)->ext_ev[0] = (c)->ext_ev[1] = nullptr;                                                       \
        } else {                                                                                             \
            hipLaunchKernelGGL(kernel, grid, block, shm, (c)->stream, __VA_ARGS__);                          \
        }                                                                                                    \
    } while (0)

// A launch that is the whole slab on the context stream (whole) goes through CDFEM_LAUNCH and takes an
// armed event pair; any other (some layers of the slab, on stream s, which may be the context stream
// too) is a plain launch and leaves the pair armed.
#define CDFEM_LAUNCH_ON(c, whole, s, kernel, grid, block, shm, ...)                                          \
    do {                                                                                                     \
        if (whole) CDFEM_LAUNCH(c, kernel, grid, block, shm, __VA_ARGS__);                                   \
        else hipLaunchKernelGGL(kernel, grid, block, shm, s, __VA_ARGS__);                                   \
    } while (0)

namespace cdfem {

// the high-order tile apply forms the point data from the affine factors; with MFMA stages
// (ho_mfma) only on the full operator (kinds 7) and the masks 1, 8, 9, else ho_mfma keeps the stream
inline bool tile_affine(const cdfem_ctx *c)
{
    if (c->d_qaff == nullptr) return false;
    if (c->ho_mfma == 0) return true;
    return c->kinds == 7 && (c->ho_mfma == 1 || c->ho_mfma == 8 || c->ho_mfma == 9);
}
// the high-order tile apply in the Kronecker form of the affine factors (k_apply3d_ktile)
inline bool tile_kron(const cdfem_ctx *c) { return c->d_qaff != nullptr && c->ho_mfma == 0 && c->pa_affine == 2; }
// the element core of the 3D p <= 2 applies (pa_core.hpp elem_apply3d_af): 0 per-point stream,
// 1 point data from the affine factors, 2 Kronecker form of the factors
inline int pa_af(const cdfem_ctx *c) { return c->d_qaff == nullptr ? 0 : (c->pa_affine == 2 ? 2 : 1); }
// pa_geom taken by the setup and still on: the 3D p <= 2 applies run the AF 3 core on d_geom
inline bool pa_geom_on(const cdfem_ctx *c) { return c->d_geom != nullptr && c->pa_geom != 0 && c->d_qaff == nullptr; }
// ho_geom taken by the setup and still on: the p = 3, 4 tile apply forms the point data from d_hgeom
// wherever it would run the stream (not the affine forms, not the matrix-core stage variants)
inline bool ho_geom_on(const cdfem_ctx *c)
{
    return c->d_hgeom != nullptr && c->ho_geom != 0 && c->d_qaff == nullptr && c->ho_mfma == 0;
}
// the form the 3D p <= 2 apply kernels are launched with (their AF argument): pa_af, or 3 under pa_geom.
// Everything else that asks for the form (folds, patch buffers, accounting of the other kernels) asks
// pa_af: AF 3 runs wherever the stream (AF 0) does, with the same launch structure.
inline int pa_form(const cdfem_ctx *c) { return pa_geom_on(c) ? 3 : pa_af(c); }
// the brick CG applies the common element matrix of a uniform box (pa_uniform: formed at the PA setup;
// set_option "pa_uniform" 0 switches back to the Kronecker form without a new setup)
inline bool uniform_elem(const cdfem_ctx *c) { return c->d_uelem != nullptr && c->pa_uniform != 0 && pa_af(c) == 2; }
// the uniform-box brick CG under Jacobi takes M^-1 from the class table (pa_uniform_diag: built and checked
// against d_dinv by ensure_dinv; set_option "pa_uniform_diag" 0 streams the vector again)
constexpr int kUdiagN = 64;
inline bool uniform_diag(const cdfem_ctx *c)
{
    return c->d_udiag != nullptr && c->dinv_ready && c->pa_uniform_diag != 0 && uniform_elem(c);
}

// ---- kernel launchers (pa_kernels.hip) -------------------------------------------------------
hipError_t launch_setup_qdata(cdfem_ctx *c, const double *d_kappa_q, const double *d_kmat_q, double kappa, double alpha,
                              const double *conv, const double *d_conv_q, const double *d_mass_q,
                              double mass);
// pa_geom: fills d_geom's blocks from the vertices (the header is the caller's)
hipError_t launch_setup_geom(cdfem_ctx *c);
// ho_geom: fills d_hgeom's elements from the vertices (the header is the caller's)
hipError_t launch_setup_hgeom(cdfem_ctx *c);
hipError_t launch_apply(cdfem_ctx *c, const double *x, double *Ye, bool constrained);
hipError_t launch_apply_wpe(cdfem_ctx *c, const double *x, double *Ye, bool con, const KrylovState *st);
hipError_t launch_apply_st(cdfem_ctx *c, const double *x, double *Ye, bool constrained,
                           const KrylovState *st);
hipError_t launch_diag_elem(cdfem_ctx *c, double *Ye);
hipError_t launch_lf_elem(cdfem_ctx *c, const double *d_fq, double *Ye);
hipError_t launch_quad_points(cdfem_ctx *c, const Rule1D &r, double *xyz);
bool apply_supported(int dim, int p);

// ---- structured brick kernels (brick_kernels.hip) --------------------------------------------
constexpr int kBrick = 4;               // elements per brick edge (4^3 = 64 = one wavefront)
constexpr int kHoBrickEdge = 2;         // p = 3, 4: elements per block edge of the high-order brick CG
bool brick_supported(int dim, int p);
int brick_count(const cdfem_ctx *c);        // bricks (p <= 2) or high-order blocks (p = 3, 4)
int brick_patch_side(const cdfem_ctx *c);   // S: 4p + 1 (p <= 2), 2p + 1 (p = 3, 4)
int brick_patch_side_z(const cdfem_ctx *c); // the patch's z side: S, or hb_ez p + 1 (p = 3, 4)
bool cg_den_fold_on(const cdfem_ctx *c);
bool cg_mr_fold(const cdfem_ctx *c);
// den partial groups of the brick CG apply at p <= 2: 1 when the bricks fit the fold bounds, else the
// power of two (<= 64) that brings them to <= kDenGroupParts sums; den_parts = the folds' partial count
constexpr int kDenGroupParts = 4096;
int den_group(const cdfem_ctx *c);
int den_parts(const cdfem_ctx *c);
constexpr int kMrFoldMaxParts = 8192;   // cg_mr_fold: apply partials every update workgroup re-sums
constexpr int kDenFoldMaxParts = 16384; // cg_den_fold: beyond (C5's 256^3 on one GPU: 262,144 bricks) the
                                        // den finalizer (the update workgroups' redundant sums grow with it)
// the Kronecker tile's x-stage table (ho_kernels.hip), built for the context's p and rule
// (its first build allocates d_ktab.  Like setup_uniform_elem, setup_uniform_diag and setup_ho_uniform_elem
// below, it reports a failed allocation by throwing HipError and any other failure by its return value; every
// caller wraps the call in HIPCHK inside guarded, so both leave as CDFEM_ERR_HIP)
hipError_t ho_ktab(cdfem_ctx *c, const double **out);
// every buffer the brick kernels reach through a 32-bit buffer resource is below c->brick_limit bytes
bool brick_fits(const cdfem_ctx *c);
// y = A x (constrained: ess in -> 0, y[ess] = x[ess]); fused E->L through LDS + face partials
hipError_t launch_brick_mult(cdfem_ctx *c, const double *x, double *y, bool constrained, int which);


// ---- vector kernels (vec_kernels.hip) --------------------------------------------------------
// y = E->L sum of Ye; constrained: y[ess] = x[ess]; if dot_part != nullptr also reduces
// partial sums of y.x into dot_part[blockIdx] and the last block writes state->den and alpha.
hipError_t launch_e2l(cdfem_ctx *c, const double *Ye, const double *x, double *y, bool constrained,
                      int cg_mode);
hipError_t launch_set_ess(cdfem_ctx *c, double *y, const double *x);          // y[ess] = x[ess]
hipError_t launch_mask_ess(cdfem_ctx *c, const double *x, double *y);        // y = x, y[ess] = 0
hipError_t launch_axpby(cdfem_ctx *c, double a, const double *x, double b, double *y);  // y = a x + b y
hipError_t launch_axpby_n(cdfem_ctx *c, int64_t n, double a, const double *x, double b, double *y);  // n entries
hipError_t launch_dinv(cdfem_ctx *c, const double *diag, double *dinv);      // 1/diag, ess -> 1
// CG pieces (MFEM CGSolver semantics)
hipError_t launch_cg_init(cdfem_ctx *c, const double *B, double *x, double *r, double *z, double *d,
                          const double *dinv, double rel_tol, double abs_tol, int max_iter);
hipError_t launch_cg_update(cdfem_ctx *c, double *x, double *r, double *z, const double *d,
                            const double *dinv);
hipError_t launch_cg_direction(cdfem_ctx *c, const double *z, double *d);
// x += alpha d, r -= alpha q, betanom = (r, M^{-1} r); z is not stored (brick path recomputes it)
hipError_t launch_cg_update_noz(cdfem_ctx *c, double *x, double *r, const double *q, const double *d,
                                const double *dinv);
hipError_t launch_zero(cdfem_ctx *c, double *y);
// one-block finalizers: den = sum(d_part[0..nparts)) (MFEM CG den step); betanom (update step)
hipError_t launch_den_fin(cdfem_ctx *c, int nparts);
hipError_t launch_update_fin(cdfem_ctx *c, int nparts, int64_t off = 0);
// brick CG v2 (brick_kernels.hip): d_new = M^{-1} r + beta d_old, q/face partials, den partials
// pa_uniform: after the PA setup of a structured p = 2 box in the Kronecker form (kinds 7 or 5), checks
// that every element's factors equal the first element's (within 1e-14 of the largest) and, if so, forms
// that element's 27 x 27 matrix (column j = the Kronecker core on e_j) in d_uelem (freed otherwise)
hipError_t setup_uniform_elem(cdfem_ctx *c);
// pa_uniform_diag: after launch_dinv on such a box (d_uelem present, one dof order), d_udiag[cx + 4 cy + 16 cz] =
// d_dinv at the lowest lattice index among the non-essential dofs of class (cx, cy, cz) (udiag_class per
// axis, brick_core.hpp); kept only if the device check finds every non-essential entry of d_dinv within
// 1e-14 (relative) of its class entry and every essential entry equal to 1 (freed otherwise)
hipError_t setup_uniform_diag(cdfem_ctx *c);
// ho_uniform: the same for a structured p = 3, 4 box whose CG runs on 2 x 2 x 4 blocks (kinds 7 or 5, one
// rank): every element's factors against element 0's, each component within 1e-14 of its own magnitude;
// if so the 64 x 64 / 125 x 125 element matrix goes to d_hoelem (freed otherwise)
hipError_t setup_ho_uniform_elem(cdfem_ctx *c);
// the option is on and the 2 x 2 x 4 block CG of one rank is taken (kinds 7 or 5): the setup's check applies;
// and the matrix is present too, so the CG apply launches k_hobrick_um
bool ho_uniform_path(const cdfem_ctx *c);
bool ho_uniform_elem(const cdfem_ctx *c);
hipError_t launch_brick_cg2(cdfem_ctx *c, const double *r, const double *dinv, const double *d_old,
                            double *d_new, double *q, double *x = nullptr, int bfkk = -1);
int cg_den_fold_grid(const cdfem_ctx *c);
bool cg_beta_fold_ok(const cdfem_ctx *c);
bool cg_beta_sum_on(const cdfem_ctx *c);
// x-fold CG after the loop: x += alpha d_m when the last update's x term is still pending
// (d_m in dbuf[(m - 1) & 1], m = the final iteration)
hipError_t launch_cg_xflush(cdfem_ctx *c, double *x, const double *d0, const double *d1);
// q from interior/face partials (+ remote interface sums), x += alpha d, r -= alpha q, betanom
hipError_t launch_cg_update_faces(cdfem_ctx *c, double *x, double *r, const double *q, const double *d,
                                  const double *dinv, const double *remote_lo, const double *remote_hi,
                                  bool den_step = false, bool xfold = false);
// generic deterministic dot into host-visible scalar via state (used by GMRES / tests)
hipError_t launch_dot(cdfem_ctx *c, const double *a, const double *b, double *d_out);
// multi-rank CG: rank-local (d, q) over owned entries into the state's den slot (all-reduce next)
hipError_t launch_den_local(cdfem_ctx *c, const double *d, const double *q);

// ---- communication (comm.hip) -----------------------------------------------------------------
void comm_destroy(cdfem_ctx *c);
void comm_allreduce(cdfem_ctx *c, double *dbuf, int n);
void comm_exchange(cdfem_ctx *c, const double *send_lo, double *recv_lo, const double *send_hi,
                   double *recv_hi, int64_t n, hipStream_t s = nullptr);
void interface_sum(cdfem_ctx *c, double *v);  // L-vector interface planes summed over ranks
// non-owned shared entries of an L-vector <- the owner's value (MFEM P applied to R v)
void interface_copy_owner(cdfem_ctx *c, double *v);
// general partition: send[off[k]..off[k+1]) -> nbr_rank[k], recv[same range] <- it (device buffers)
void comm_exchange_nbr_buf(cdfem_ctx *c, const std::vector<int64_t> &off, const double *dsend, double *drecv,
                           hipStream_t s = nullptr);
void partition_free(cdfem_ctx *c);
inline bool multi_rank(const cdfem_ctx *c) { return c->nranks > 1; }
// split CG finalizers for the multi-rank path: local sum -> all-reduce -> step
hipError_t launch_fin_sum(cdfem_ctx *c, int nparts, int slot);
hipError_t launch_den_step(cdfem_ctx *c);
hipError_t launch_update_step(cdfem_ctx *c);
hipError_t launch_init_step(cdfem_ctx *c, double rel_tol, double abs_tol, int max_iter);
hipError_t launch_cg_init_nofin(cdfem_ctx *c, const double *B, double *x, double *r, double *z, double *d,
                                const double *dinv);
// pack the local partial sums of q on the shared interface planes into d_if[0] / d_if[2]
hipError_t launch_pack_qplanes(cdfem_ctx *c, const double *q, hipStream_t s = nullptr);
hipError_t launch_brick_cg2_split(cdfem_ctx *c, const double *r, const double *dinv, const double *d_old,
                                  double *d_new, double *q, hipStream_t s, double *x = nullptr, int bfkk = -1);

// ---- bandwidth probes (stream_kernels.hip): mode 0 read 16 B/lane, 1 read 8 B/lane, 2 copy 16 B
// full assembly on simplices (fa_kernels.hip)
constexpr int kSpmvMaxBlocks = 65536;  // partial slots reserved for the SpMV-CG den
constexpr int kLdsHaloMax = 7936;      // doubles of x one LDS-staged SpMV window may stage (62 KiB)
struct FaPattern {
    int64_t nnz = 0;
    std::vector<int32_t> rowptr, cols, diagpos, coff, cpos;
    // SELL-64 (sigma = global sort by row length) copy of the pattern for the SpMV
    std::vector<int32_t> sptr;   // [nslices + 1] first stored entry of each 64-row slice
    std::vector<int32_t> srows;  // [nslices * 64] original row of (slice, lane), -1 = padding
    std::vector<int32_t> scols;  // [stored] column, slice-major then entry-major then lane
    std::vector<int32_t> smap;   // [stored] CSR index of the stored entry, -1 = padding
    std::vector<int16_t> sdel;   // [stored] column - lane row where it fits 16 bits (see swide), else empty
    std::vector<uint8_t> swide;  // [nslices] 1: this slice has a delta beyond 16 bits and streams scols
                                 // (empty: every slice fits); nnz_wide = real entries in such slices
    int64_t nnz_wide = 0;
    // LDS-staged windows (windowed layouts, sell_build with lds_rows > 0): window w = slices
    // [w S, (w + 1) S), S = lds_rows / 64; its distinct columns hidx[hptr[w] .. hptr[w + 1]) (ascending)
    // are staged in LDS and every stored entry addresses them by sloc (16-bit position in the window)
    int64_t lds_rows = 0;
    int lpr = 1;                  // lanes per row (R = 64 / lpr rows per slice; LDS layouts only)
    int32_t lds_max = 0;          // largest window halo (doubles of LDS)
    std::vector<int32_t> hptr, hidx;
    std::vector<uint16_t> sloc;
    std::vector<int32_t> perm;   // SpMV space order (sell_plan.cpp): space row -> mesh row; empty = mesh order
    bool windowed = false;       // slices cut from the space order directly (no srows)
};
// SpMV order (sell_plan.cpp): 0 natural + global sort, 1 natural + windows, 2 RCM + windows,
// 3 auto (mode 0, geometric or RCM + global), 4 RCM + global, 5 geometric + global
struct SellPlan {
    int mode = 0, base = 1;  // base: 1 natural, 2 RCM, 3 geometric, 4 Morton
    bool windowed = false;
    int64_t window = 0, max_delta = 0, bw_natural = 0, bw_rcm = 0, bw_geometric = 0;
    std::vector<int32_t> perm;   // space row -> mesh row (empty: mesh order)
    int64_t lds_rows = 0;        // windowed: rows per LDS-staged window (set_option "spmv_lds"; 0 off)
    bool auto_lds = false;       // the auto mode chose a windowed unstructured order: LDS windows
    int lpr = 1;                 // LDS layouts: lanes per row (set_option "spmv_lpr")
};
constexpr int64_t kAutoLdsRows = 768;  // rows per window of the auto LDS orders (profiles/r03/ab_c4_lds_windows.txt)
std::vector<int32_t> rcm_order(int64_t nl, const int32_t *rowptr, const int32_t *cols);
SellPlan sell_plan(int64_t nl, const int32_t *rowptr, const int32_t *cols, int mode, int dim = 0,
                   const double *xyz = nullptr, int64_t window = 0);
// dof coordinates of a simplex space (P1, P2, triangle P3 nodes; element-affine map), nl * dim
std::vector<double> simplex_dof_coords(int dim, int p, int ne, int nd, int64_t nl, const std::vector<double> &verts,
                                       const std::vector<int32_t> &dofs);
// dof coordinates of a quad / hex space: the multilinear map of the element's 2^dim vertices at the GLL nodes
std::vector<double> tensor_dof_coords(int dim, int p, int ne, int nd, int64_t nl, const std::vector<double> &verts,
                                      const std::vector<int32_t> &dofs);
void sell_build(FaPattern &P, int64_t nl, const SellPlan &pl);
FaPattern fa_build_pattern(const std::vector<int32_t> &elem_dofs, int ne, int nd, int64_t nl, int sell_mode,
                           int dim = 0, const double *dof_xyz = nullptr, int64_t sell_window = 0,
                           int64_t lds_rows = 0, int lpr = 1);
// f(DIM, P) as constants for the simplex spaces: tetrahedra of p = 1, 2, triangles of p = 1, 2, 3
template <class F>
hipError_t dispatch_simplex(const cdfem_ctx *c, F &&f)
{
    if (c->p < 1 || c->p > 3) return hipErrorInvalidValue;
    return dispatch_value<31, 32, 21, 22, 23>(10 * c->dim + c->p, hipErrorInvalidValue, [&](auto DP) {
        return f(std::integral_constant<int, DP() / 10>{}, std::integral_constant<int, DP() % 10>{});
    });
}
hipError_t launch_simplex_elem(cdfem_ctx *c, const double *kq, const double *kmq, double kappa, double alpha,
                               const double *conv, const double *cq, const double *mq, double mass);
// the same on quads p = 1..4 and hexes p = 1, 2 (fa_tensor.hip): k_tensor_elem on the OPERATOR rule, element e the
// mesh-order element (structured contexts too); per-point arrays in cdfem_quadrature_points(CDFEM_RULE_OPERATOR)'s order
bool fa_tensor_supported(int dim, int p);
hipError_t launch_tensor_elem(cdfem_ctx *c, const double *kq, const double *kmq, double kappa, double alpha,
                              const double *conv, const double *cq, const double *mq, double mass);
hipError_t launch_fa_assemble(cdfem_ctx *c);
hipError_t launch_simplex_lf(cdfem_ctx *c, const double *fq, double *Ye);
hipError_t launch_sell_fill(cdfem_ctx *c);
hipError_t launch_csr_diag(cdfem_ctx *c, double *d);
hipError_t launch_spmv(cdfem_ctx *c, bool constrained, const double *x, double *y);
hipError_t launch_spmv_cg(cdfem_ctx *c, const double *d, double *q);
// permuted SpMV layout: dst = src gathered into the SpMV order (to_spmv_order) or scattered back
hipError_t launch_perm(cdfem_ctx *c, bool to_spmv_order, const double *src, double *dst);
bool spmv_delta(const cdfem_ctx *c);
// fused high-order CG iteration (ho_kernels.hip / vec_kernels.hip)
bool tile_den_ok(const cdfem_ctx *c);
int tile_den_blocks(const cdfem_ctx *c, bool most = false);
hipError_t launch_apply_den(cdfem_ctx *c, const double *d, double *Ye, const KrylovState *st, double *part);
// the same with the CG direction folded in (ho_dfold, Kronecker tile): d_new = z + beta d_old
bool tile_dfold_ok(const cdfem_ctx *c);
hipError_t launch_apply_den_dfold(cdfem_ctx *c, const double *z, const double *dold, double *dnew, double *Ye,
                                  const KrylovState *st, double *part);
bool e2l_box_ok(const cdfem_ctx *c);
hipError_t launch_den_from_partials(cdfem_ctx *c, const double *in, int64_t n);
hipError_t launch_den_local_from_partials(cdfem_ctx *c, const double *in, int64_t n);
hipError_t launch_e2l_cg_update(cdfem_ctx *c, const double *Ye, const double *d, double *x, double *r, double *z,
                                const double *dinv);

// GMRES(m) (gmres.hip)
int gmres_blocks(int64_t n);
hipError_t launch_gm_init(cdfem_ctx *c, GmresState *st, int m, int max_it);
// poll: pinned host slot the step's last scalar kernel writes the state head into (solve_gmres)
hipError_t launch_gm_residual(cdfem_ctx *c, const double *b, const double *Ax, const double *dinv, double *v0,
                              double *part, GmresState *st, bool first, double rtol, double atol, GmresHead *poll);
// ps (gm_pb): pass 1 reads the structured Mult's patch buffer for A_c V_j instead of w (brick_core.hpp)
struct GmPatchSrc;
hipError_t launch_gm_orth(cdfem_ctx *c, double *w, const double *dinv, double *V, int64_t ldv, double *part,
                          GmresState *st, int m, GmresHead *poll, const GmPatchSrc *ps = nullptr);
hipError_t launch_gm_update(cdfem_ctx *c, double *x, const double *V, int64_t ldv, GmresState *st, GmresHead *poll);

// BiCGStab (bicgstab.hip); ps as for launch_gm_orth: k_bcgs_v / k_bcgs_t read the patch buffer instead of w
int bcgs_blocks(int64_t n);
hipError_t launch_bcgs_init(cdfem_ctx *c, const double *b, const double *dinv, double *r, double *rh, double *part,
                            BcgsState *st, double rtol, double atol, int max_it, BcgsHead *poll);
hipError_t launch_bcgs_p(cdfem_ctx *c, const double *r, double *p, const double *v, BcgsState *st);
hipError_t launch_bcgs_v(cdfem_ctx *c, const double *w, const double *dinv, const double *rh, double *v, double *r,
                         double *part, BcgsState *st, const GmPatchSrc *ps = nullptr);
hipError_t launch_bcgs_t(cdfem_ctx *c, const double *w, const double *dinv, double *x, const double *p, double *r,
                         double *t, const double *rh, double *part, BcgsState *st, BcgsHead *poll,
                         const GmPatchSrc *ps = nullptr);
hipError_t launch_stream(cdfem_ctx *c, int mode, const double *a, double *b, int64_t n);
// ILU(0) (ilu_kernels.hip): factor + capture once per operator; apply: ilu.z = (LU)^{-1} d_w[4]
void ilu_setup(cdfem_ctx *c);
void ilu_free(cdfem_ctx *c);
hipError_t ilu_apply(cdfem_ctx *c);
// f64 compute-rate probes: mode 0 VALU v_fma_f64, 1 v_mfma_f64_16x16x4_f64; *flops per launch
hipError_t launch_fp64_probe(cdfem_ctx *c, int mode, double *out, double *flops);

// ---- the nonlinear heat form (nl_kernels.hip; the Newton driver and the entry points: newton.hip) ----
// dofs of the facet opposite local vertex f in the element's local dof order (vertices, then edge nodes):
// row (space, f) of the table, spaces in the order triangles P1, P2, P3, tetrahedra P1, P2
constexpr int kFacetMaxDofs = 6;
__host__ __device__ constexpr int facet_space(int dim, int p) { return dim == 2 ? p - 1 : 2 + p; }
__host__ __device__ constexpr int facet_ndofs(int dim, int p) { return dim == 2 ? p + 1 : (p + 1) * (p + 2) / 2; }
__host__ __device__ constexpr int facet_dof(int dim, int p, int f, int k)
{
    constexpr int8_t t[5][4][kFacetMaxDofs] = {
        {{1, 2}, {0, 2}, {0, 1}},
        {{1, 2, 5}, {0, 2, 4}, {0, 1, 3}},
        {{1, 2, 7, 8}, {0, 2, 5, 6}, {0, 1, 3, 4}},
        {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}},
        {{1, 2, 3, 7, 8, 9}, {0, 2, 3, 5, 6, 9}, {0, 1, 3, 4, 6, 8}, {0, 1, 2, 4, 5, 7}}};
    return t[facet_space(dim, p)][f][k];
}
// Ye (element-major E-vector) = the residual's element vectors at u, with u_old from c->nl
hipError_t launch_nl_residual(cdfem_ctx *c, const double *u, double *Ye);
// d_Ee = the Jacobian's element matrices at u (k_simplex_elem's layout)
hipError_t launch_nl_gradient(cdfem_ctx *c, const double *u);
// R = ess ? 0 : R - g; negR (may be null) = -R
hipError_t launch_nl_finish(cdfem_ctx *c, double *R, const double *g, double *negR);
// facet E-vector from the point values gq, then b = its per-dof sums in ascending facet order
hipError_t launch_bdr_lf(cdfem_ctx *c, const double *gq, double *b);
inline cdfem_nl_heat_coeffs nl_coeffs(const cdfem_ctx *c)
{
    return cdfem_nl_heat_coeffs{c->heat.dt, c->heat.a0, c->heat.a1, c->heat.m0, c->heat.m1, c->heat.u_ref};
}
// the same form on quads and hexes (nl_tensor.hip, nl_fa_tensor.hip, the boundary form's faces): the spaces it is
// built for (quads of p = 1..3, hexes of p = 1, 2), f(DIM, P) as constants for them, and its rule's points per
// direction
bool nl_tensor_supported(int dim, int p);
template <class F>
hipError_t dispatch_nl_tensor(const cdfem_ctx *c, F &&f)
{
    return dispatch_value<21, 22, 23, 31, 32>(10 * c->dim + c->p, hipErrorInvalidValue, [&](auto DP) {
        return f(std::integral_constant<int, DP() / 10>{}, std::integral_constant<int, DP() % 10>{});
    });
}
__host__ __device__ constexpr int nl_tensor_points_1d(int dim, int p) { return dim == 3 ? p + 3 : p + 2; }
// matrix-free: k_nl_tensor in mode 0 (Ye = the elements' shares of R(u)), 1 (of J(u) v; con: essential entries of
// v read as 0) or 2 (of J(u)'s diagonal), Ye in the context's E-vector layout; u_old from c->heat
hipError_t launch_nl_tensor(cdfem_ctx *c, int mode, const double *u, const double *v, bool con, double *Ye,
                            const KrylovState *st);
// with the Jacobian assembled (nl_fa_tensor.hip): the doubles of the point state c->heat.d_jq, and d_Ee = the
// element matrices of J(u) (k_nl_tensor_point, then k_nl_tensor_elem)
size_t nl_fa_tensor_state_size(const cdfem_ctx *c);
hipError_t launch_nl_tensor_elem(cdfem_ctx *c, const double *u);
// the facet E-vector of the boundary linear form on quad / hex faces (k_bdr_lf_tensor; launch_bdr_lf gathers it)
hipError_t launch_bdr_lf_tensor(cdfem_ctx *c, const double *gq);
// the matrix-free Jacobian of the nonlinear form is the current operator: every structured fast path of the
// linear operator is off (they key on the mesh), and the launch points route to k_nl_tensor
inline bool nl_jac_current(const cdfem_ctx *c) { return c->heat.jac_mf; }
// the assembled operator's pattern on the device, built once per mesh (capi.hip; cdfem_fa_setup, cdfem_nl_gradient)
void fa_ensure_pattern(cdfem_ctx *c);

// ---- the operator and the Krylov drivers (solve.hip), the cost model (model.hip) ----------------
bool use_brick(const cdfem_ctx *c);       // the p <= 2 brick kernels run the structured Mult and CG
bool use_hobrick_cg(const cdfem_ctx *c);  // the p = 3, 4 block CG runs
bool use_brick_cg(const cdfem_ctx *c);    // either
void op_apply(cdfem_ctx *c, const double *x, double *y, bool constrained);         // rank-local
void op_apply_global(cdfem_ctx *c, const double *x, double *y, bool constrained);  // + shared dofs summed
void ensure_dinv(cdfem_ctx *c);           // d_dinv (and the pa_uniform_diag table) formed once per operator
// the Krylov driver p.method and the context select; dB, dX on the device, in the solve's order
void solve(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *dX, cdfem_solver_result &res);
// what cdfem_solve refuses in its parameters (ArgError / UnsupportedError)
void check_solver_params(const cdfem_solver_params &p);
// solve with dB, dX in the mesh's dof order: under a permuted SpMV layout the Krylov iteration runs in the
// SpMV's order, B in and X out permuted once per solve
void solve_mesh_order(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *dX, cdfem_solver_result &res);
inline int nq_of(const cdfem_ctx *c, const Rule1D &r) { return c->dim == 3 ? r.q1 * r.q1 * r.q1 : r.q1 * r.q1; }
void kernel_name(const cdfem_ctx *c, int k, char *buf, size_t n);
double kernel_flops(const cdfem_ctx *c, int k);
double kernel_bytes(const cdfem_ctx *c, int k);

}  // namespace cdfem
