// ctx_state.hpp — the parts of cdfem_ctx that live as long as one uploaded mesh (MeshState) or one declared
// rank partition (PartitionState).  Both are reset by assigning a default-constructed one, which frees every
// buffer and puts every flag back to its initialiser: a field added here needs no line anywhere else.
// No HIP header (tests/cpp/ctx_state_check.cpp compiles this with the host compiler).
#pragma once
#include <cstdint>
#include <vector>

#include "handles.hpp"

namespace cdfem {

constexpr int kMaxD1 = 6;
constexpr int kMaxQ1 = 8;

// 1D tables for one quadrature rule: B[q][d] = phi_d(xi_q), G[q][d] = phi_d'(xi_q), points, weights
struct Rule1D {
    int d1 = 0, q1 = 0;
    double B[kMaxQ1][kMaxD1] = {};
    double G[kMaxQ1][kMaxD1] = {};
    double pts[kMaxQ1] = {};
    double wts[kMaxQ1] = {};
};

// The assembled operator's pattern on the device (cdfem_fa_setup, once per mesh): CSR with sorted columns,
// deterministic contribution lists, and the SELL-64 copy the SpMV streams.  A struct of its own so that the
// setup builds one aside and moves it into the context whole: a refused setup leaves no half-built pattern.
struct FaDeviceState {
    int64_t nnz = 0;
    DevBuf<int32_t> d_rowptr, d_cols, d_diagpos;
    DevBuf<int32_t> d_coff, d_cpos;     // per-nonzero contribution lists into d_Ee
    DevBuf<double> d_vals;              // A
    DevBuf<double> d_vals_c;            // eliminated A (FormLinearSystem, DIAG_ONE)
    DevBuf<double> d_Ee;                // element matrices [blk][nd*nd][64]
    int64_t nslices = 0, nstored = 0;   // SELL-64 copy (the SpMV layout)
    DevBuf<int32_t> d_sptr, d_srows, d_scols, d_smap;
    DevBuf<int16_t> d_sdel;             // 16-bit column deltas (null when the bandwidth does not fit)
    DevBuf<uint8_t> d_swide;            // per slice: 1 = streams 32-bit columns (mixed layout; null: none)
    int64_t sell_nnz_wide = 0;          // real entries in the 32-bit slices of a mixed layout
    DevBuf<int32_t> d_hptr, d_hidx;     // LDS-staged windows (FaPattern::hptr / hidx / sloc)
    DevBuf<uint16_t> d_sloc;
    int64_t lds_rows = 0;               // rows per window of the current LDS layout (0: none)
    int32_t lds_max = 0;                // largest window halo (doubles)
    int sell_lpr = 1;                   // lanes per row of the current SELL copy
    DevBuf<int32_t> d_rperm;            // SpMV space order: space row -> mesh row (null: mesh order)
    bool sell_windowed = false;         // slices cut from the space order (kernel row = slice * 64 + lane)
    DevBuf<double> d_pv[2];             // permuted-space scratch (apply in mesh order; solve B / X)
    DevBuf<double> d_svals, d_svals_c;
};

// The nonlinear heat form and its Newton solve (cdfem_nl_setup, cdfem_bdr_set; nl_kernels.hip, newton.hip):
// coefficients, the tables of the order 2p + 2 rule, the boundary facets with their rule and gather lists,
// the Newton vectors (device-resident for a whole solve) and the history of the last solve.
// On quad / hex meshes (cdfem_nl_pa_setup; nl_tensor.hip) the form is matrix-free: the tensor rule's 1D tables,
// and the Jacobian as the state it was linearised at.  cdfem_nl_fa_setup (nl_fa_tensor.hip) keeps the residual
// matrix-free and assembles the Jacobian into the full assembly's CSR, through the point state d_jq.
struct NlState {
    bool ready = false;
    bool tensor = false;                // set up by cdfem_nl_pa_setup or cdfem_nl_fa_setup (quads / hexes)
    bool assembled = false;             // tensor, by cdfem_nl_fa_setup: cdfem_nl_gradient assembles J(u)
    bool jac_mf = false;                // the matrix-free J(d_ulin) is the context's current operator
    Rule1D rule;                        // tensor: Gauss-Legendre, p + 2 (quads) / p + 3 (hexes) points per direction
    DevBuf<double> d_ulin;              // tensor: the linearisation state, a copy (the Newton loop updates d_u in place)
    DevBuf<double> d_jq;                // assembled: a(u), mu, grad u at the points, [nblk][nq][2 + dim][64] (kept across rebuilds)
    double dt = 0.0, a0 = 0.0, a1 = 0.0, m0 = 0.0, m1 = 0.0, u_ref = 0.0;
    int nq = 0;                         // points of the order 2p + 2 rule
    std::vector<double> h_sxi;          // its points (reference coordinates)
    DevBuf<double> d_tab;               // phi [nq][nd], dphi [nq][nd][dim], w [nq]
    DevBuf<int32_t> d_edofs;            // [ne][nd] element dofs, element-major
    DevBuf<double> d_u, d_R, d_rhs, d_dx;  // Newton iterate, residual, -residual, update
    DevBuf<double> d_uold, d_g;         // u of the last step; the Neumann load (zero when unset)
    DevBuf<double> d_norm;              // [1] a norm's square on its way to the host
    // boundary linear form (cdfem_bdr_set)
    int nbf = 0, nqb = 0, nfd = 0;      // facets, points per facet, dofs per facet
    int nqb1 = 0;                       // quad / hex faces: points per direction of the facet rule
    std::vector<int32_t> h_face_elem, h_face_local;
    std::vector<double> h_bxi;          // [dim + 1][nqb][dim] facet points in the element's reference coordinates
                                        // (quad / hex faces: [2 dim][nqb][dim])
    std::vector<double> h_bverts;       // quad / hex faces: [nbf][2^dim][dim] vertices of the facets' elements
    DevBuf<int32_t> d_face_elem, d_face_local;
    DevBuf<double> d_btab;              // phi [dim + 1][nqb][nfd] of the facet's dofs, w [nqb]
                                        // (quad / hex faces: B [nqb1][p + 1], pts [nqb1], w [nqb1] of the 1D rule)
    DevBuf<int32_t> d_b_off, d_b_pos;   // per dof: its entries of the facet E-vector, ascending facet
    DevBuf<double> d_bYe, d_bgq;        // facet E-vector [nbf][nfd]; point values [nbf][nqb]
    // per-iteration history of the last Newton solve
    std::vector<double> hist_res, hist_upd;
    std::vector<int32_t> hist_lin;
};

// Everything cdfem_mesh_upload / cdfem_mesh_upload_simplex start from scratch.  (The mesh's sizes, rules and
// host copies are assigned by every upload before mesh_ready and stay in ContextState.)
struct MeshState : FaDeviceState {
    bool mesh_ready = false;
    DevBuf<double> d_verts;             // [ne][nv][dim]
    DevBuf<int32_t> d_map;              // [nblk][nd][64], ess negative
    DevBuf<int32_t> d_e2l_off;          // [nl+1]
    DevBuf<int32_t> d_e2l_pos;          // [ne*nd]
    DevBuf<uint8_t> d_ess;              // [nl]
    DevBuf<int32_t> d_ess_list;         // [n_ess]
    DevBuf<int32_t> d_perm;             // [nblk*64] element at (block, lane), -1 = padding

    // structured-box fast path (cdfem_mesh_set_structured): 4x4x4-element bricks
    bool structured = false;
    bool epencil = false;               // qlay 1 on a structured box: pencil E-vector layout (ho_eidx)
    int hb_nblk = 0;                    // blocks of the high-order brick CG (hb_nbx * hb_nby * hb_nbz)
    DevBuf<uint8_t> d_bess;             // per brick (block): 1 if a dof of its patch is essential
    DevBuf<double> d_hbpart;            // den partials summed in two stages: k_hobrick_cg's, and k_brick_cg's past
                                        // kDenFoldMaxParts bricks on one rank (one per brick)
    // grouped den partials (p <= 2 past the fold bounds: C5's per-rank slab of 32,768 bricks, its 262,144 on one
    // GPU): the last-arriving brick of each group of den_grp sums the group's partials in a fixed order
    // (k_brick_cg tail: write-through partial, agent-scope arrival count), so the folds sum <= 4,096 values
    int den_grp = 1;                    // group size of the running solve (1: one partial per brick)
    DevBuf<double> d_gsum;              // [ceil(nblk / den_grp)] group sums
    DevBuf<uint32_t> d_gcnt;            // [same] arrival counters (0 between launches)
    DevBuf<double> d_uelem;             // pa_uniform: the common element matrix in MFMA A-operand order
    DevBuf<double> d_udiag;             // [kUdiagN] the class table (setup_uniform_diag, valid while dinv_ready;
                                        // null when the device check found d_dinv not class-constant)
    DevBuf<double> d_hoelem;            // ho_uniform: that matrix in MFMA A-operand order ([row tile][k step][lane],
                                        // zero-padded to 16 x 4 multiples: 128 x 128 at p = 4)
    DevBuf<double> d_face;              // [nblk][F] brick-face partial sums
    DevBuf<double> d_ones;              // all-ones vector (unpreconditioned brick CG)
    DevBuf<double> d_dalt;              // second search-direction buffer (brick CG)
    // slab partition: the largest L-vector and brick count over all ranks (all-reduced by cdfem_set_slab),
    // so brick_fits takes the same decision on every rank (slabs of different sizes near the
    // bound would otherwise send ranks down CG paths with different collective sequences)
    int64_t slab_nl_max = 0, slab_nb_max = 0;
    int zlo_shared = 0;                 // local gz=0 plane owned by the rank below (slabs)
    int zhi_shared = 0;                 // local gz=Lz-1 plane shared with the rank above
    DevBuf<double> d_if[4];             // interface planes: send_lo, recv_lo, send_hi, recv_hi

    // geometry family: 0 tensor (quad/hex: PA), 1 simplex (tri/tet: FA, cdfem_mesh_upload_simplex)
    int geom = 0;
    DevBuf<double> d_stab;              // rule tables, diffusion rule first then the convection + mass
                                        // rule, each phi [nq][nd], dphi [nq][nd][dim], w [nq]
    std::vector<double> h_verts;        // simplex host geometry (quadrature points for coefficients)
    std::vector<double> h_sxi_d, h_sxi_cm;  // the two rules' points (reference coordinates)
    std::vector<double> h_sxi_lf;       // simplex LINEARFORM rule (collapsed Gauss, n = p + 3)
    DevBuf<double> d_stab_lf;           // phi [nq_lf][nd], w [nq_lf]
    bool fa_ready = false;              // full assembly (cdfem_fa_setup): FaDeviceState filled and assembled
    DevBuf<double> d_tpart;             // den partials of the fused high-order CG apply (one per tile block)
    DevBuf<double> d_ktab;              // k_apply3d_ktile's rows of M, K, C, C^T (canonical entries, [4][D1][D1])
    int ktab_key = -1;                  //   (p, rule) the table was built for; -1: rebuilt by the next launch
    DevBuf<double> d_bsum;              // [2] cg_beta_sum: the betanom sum, then the update's arrival counter (0 between launches)
    DevBuf<double> d_small;             // a few doubles of device scratch (mr_fold_agreed's all-reduce)
    DevBuf<double> d_dinv_p;            // the Jacobi scale in permuted order (during such a solve)

    // partial assembly
    bool pa_ready = false;
    DevBuf<double> d_qd;                // [nblk][nq][nc][64]
    DevBuf<double> d_qaff;              // [nblk][nc][64] per-element factors of an affine mesh (qd = W_q * g)
    DevBuf<double> d_geom;              // pa_geom: header + [nblk][22][64] masks and map coefficients (GeomLayout)
    DevBuf<double> d_hgeom;             // ho_geom: GeomLayout's header + [ne][24] map coefficients (HoGeomLayout)
    DevBuf<double> d_Ye;                // [nblk][nd][64]
    DevBuf<double> d_dinv;              // Jacobi (constrained: ess -> 1)
    bool dinv_ready = false;

    // work vectors (L-size); the solvers' own are allocated by the first solve that needs them
    DevBuf<double> d_w[8];              // staging + Krylov vectors
    DevBuf<double> d_part;              // reduction partials [red_blocks + nblk]
    DevBuf<double> d_gm;                // GMRES basis (restart+1) * padded nl
    DevBuf<double> d_gm_part;           // GMRES partials [(restart+1) * blocks]
    DevBuf<double> d_lfq;               // cdfem_lf_assemble: the point values (kept across calls)
    DevBuf<double> d_bcgs;              // BiCGStab vectors x, r, rh, p, v, t (6 * padded nl)
    DevBuf<double> d_bcgs_part;         // BiCGStab partials [3 * blocks]
    NlState heat;                       // the nonlinear heat form (cdfem_nl_setup)
};

// The rank partition of the L-vector (cdfem_set_slab / cdfem_set_shared), reset by partition_free
struct PartitionState {
    // 0 none, 1 z-slab (cdfem_set_slab), 2 general element partition (cdfem_set_shared).  Both number the
    // dofs owned by a lower rank first, so the owned (true) dofs are the suffix [skip_lo, nl) and every dot
    // product skips the prefix.
    int part_mode = 0;
    int64_t skip_lo = 0;
    // general partition: per neighbour rank (ascending) the shared local dofs, same order on both
    // sides; send/recv buffers concatenated in neighbour order
    std::vector<int32_t> nbr_rank;
    std::vector<int64_t> nbr_off;       // [n_nbr + 1]
    std::vector<int32_t> h_sh_idx;      // [n_sh] local dof of send/recv slot (host copy)
    DevBuf<int32_t> d_sh_idx;           // [n_sh] local dof of send/recv slot
    DevBuf<double> d_sh_send, d_sh_recv;
    int32_t n_shd = 0;                  // distinct shared dofs
    DevBuf<int32_t> d_shd;              // [n_shd] their local index
    DevBuf<int32_t> d_shd_off;          // [n_shd + 1] contributions, ascending rank (own = -1)
    DevBuf<int32_t> d_shd_src;          //   source: -1 own partial, else recv slot
    DevBuf<int32_t> d_shd_owner;        // [n_shd] recv slot of the owner's copy, -1 if owned here
};

}  // namespace cdfem
