// options.hpp — every cdfem_set_option switch: the field with its default (cdfem::Options, the base of
// cdfem_ctx), and one table row per key with the values it accepts and the text of its refusal.
// Host only, no HIP: tests/cpp/options_check.cpp checks the table on its own.
#pragma once
#include <climits>
#include <cstdint>
#include <cstring>
#include <string>

namespace cdfem {

struct Options {
    // ---- structured boxes: the p = 2 brick CG and the p = 3, 4 block CG --------------------------
    int brick_xcd = 1;                  // k_brick_cg brick order: 0 dispatch, 1 XCD-contiguous (default)
    // the brick kernels address r, M^-1, d, x, ess and the patch buffer through buffer resources with
    // 32-bit byte offsets and the out-of-range marker kOOB = 2^31, so every such buffer must stay below
    // 2^31 bytes (8 N_L and 8 S^3 nblk); larger boxes take the generic 64-bit-indexed element kernels.
    // set_option "brick_byte_limit" lowers the bound (tests force the fallback on small boxes).
    int64_t brick_limit = (int64_t)1 << 31;
    int den_group_opt = 0;              // set_option "den_group": 0 automatic, else this group size (tests)
    int brick_stagger = -1;             // set_option "brick_stagger": BrickGeom::stag (-1 automatic, 0 off)
    int brick_mfma = 0;                 // set_option "brick_mfma": k_brick_cg's x stage on the matrix cores (p = 2, kinds 7)
    int pa_uniform = 1;                 // set_option "pa_uniform": when every element's factors equal the first
                                        // element's (a uniformly refined box, what MFEM's MakeCartesian3D
                                        // gives), the p = 2 brick CG applies that element's 27 x 27 matrix on
                                        // the matrix cores (brick_um.hip k_brick_cg<XF, BF, FULL>); 0 keeps the Kronecker form
    int pa_uniform_diag = 1;            // set_option "pa_uniform_diag": with pa_uniform, the Jacobi-CG apply and update take
                                        // M^-1 from the 64 lattice-class values of d_udiag instead of streaming d_dinv
    int brick_mult_pb = 1;              // set_option "brick_mult_pb": structured Mult through the patch buffer
    int brick_upd_pb = 1;               // set_option "brick_upd_pb": predicated-load face sums in the brick CG update
    int mr_overlap = 1;                 // set_option "mr_overlap": slab CG exchange overlapped with interior bricks
    int cg_beta_fold = 1;               // set_option "cg_beta_fold": brick CG betanom step in the next apply
    int cg_beta_sum = 0;                // set_option "cg_beta_sum": with it, on one rank before the uniform-box apply, the
                                        // update's last workgroup sums the betanom partials once (cg_beta_sum_on);
                                        // off: measured slower (profiles/r14/ab_c2_one_round/)
    int cg_mr_fold = 1;                 // set_option "cg_mr_fold": both folds on several ranks (partials all-reduced)
    int cg_den_fold = 1024;             // set_option "cg_den_fold": brick CG den step in the update (N workgroups; 0 off)
    int cg_xfold = 1;                   // set_option "cg_xfold": brick CG folds x += alpha d into the next apply
    int ho_block_z = 2;                 // set_option "ho_block_z": elements per block along z (2 or 4), read by
                                        // cdfem_mesh_set_structured; 4 = 2 x 2 x 4 blocks
    int ho_brick = 1;                   // set_option "ho_brick": high-order CG through k_hobrick_cg + the brick update
    int ho_brick_mfma = 0;              // set_option "ho_brick_mfma": its x stage on v_mfma_f64_16x16x4_f64 (kinds 7)
    int ho_uniform = 0;                 // set_option "ho_uniform": the p = 3, 4 block CG (2 x 2 x 4 blocks) applies the
                                        // common N x N element matrix of a uniform box (N = 64, 125) as one GEMM on
                                        // the matrix cores (k_hobrick_um); read by cdfem_pa_setup, 0 afterwards
                                        // switches back to the Kronecker form without a new setup
    int ho_uniform_grid = 0;            // set_option "ho_uniform_grid": k_hobrick_um's workgroups (0 automatic; tests)

    // ---- the generic high-order CG ----------------------------------------------------------------
    int ho_dfold = 1;                   // set_option "ho_dfold": CG direction folded into the Kronecker tile apply
    int ho_mfma = 0;                    // set_option "ho_mfma": bit 0 = stage x of the p >= 3 tile apply on MFMA
    int cg_fused = 1;                   // set_option "cg_fused": fused high-order CG iteration (p >= 3 boxes)

    // ---- partial assembly ---------------------------------------------------------------------------
    int pa_affine = 2;                  // set_option "pa_affine": when the mesh allows, 1 form the point data
                                        // from the affine factors, 2 the Kronecker form of the same factors
                                        // (3D p <= 2 applies; the p >= 3 tile apply takes 2 as 1); 0 stream
    int pa_geom = 0;                    // set_option "pa_geom": 1 = on a hex mesh the affine forms do not take (3D
                                        // p <= 2, constant coefficients) the applies form the point data from the
                                        // element's trilinear map (AF 3) instead of streaming it; read by
                                        // cdfem_pa_setup, 0 afterwards switches back to the stream
                                        // (3D hex p <= 2 applies k_apply3d, k_brick3d, k_brick_cg; the p = 3, 4
                                        // tile kernels and the 2D applies keep the stream)
    int ho_geom = 0;                    // set_option "ho_geom": the same for the 3D p = 3, 4 tile apply where it runs
                                        // the stream (MF & 32 of k_apply3d_tile, ho_mfma 0); read by cdfem_pa_setup,
                                        // 0 afterwards switches back to the stream

    // ---- GMRES and BiCGStab -------------------------------------------------------------------------
    int gm_ept = 0;                     // set_option "gm_ept": GMRES orthogonalisation entries per thread (0: auto, orth_ept)
    int gm_pb = 1;                      // set_option "gm_pb": GMRES pass 1 reads the structured Mult's patch buffer
    int gm_poll = 4;                    // set_option "gm_poll": the host polls the GMRES state every k inner steps

    // ---- the assembled SpMV (all but the last two read when the FA pattern is built, once per mesh) --
    int sell_mode = 8;                  // set_option "sell_order"
    int sell_window = 0;                // set_option "sell_window": rows per window of a windowed order (0 auto)
    int spmv_lds = -1;                  // set_option "spmv_lds": rows per LDS-staged SpMV window (0 off, -1 auto)
    int spmv_lpr = 0;                   // set_option "spmv_lpr": lanes per row of the LDS layouts (0 auto, 1, 2, 4)
    int spmv_xcd = 1;                   // set_option "spmv_xcd": contiguous slice range per XCD (windowed layout)
    int spmv_index16 = 1;               // set_option "spmv_index16": SpMV streams d_sdel when present

    unsigned prof_mask = ~0u;           // kernels that get HIP events while profiling (set_option profile_mask)
};

// the values a key accepts: a 0/1 flag, a closed range, a short list, or (written in the row) a predicate
template <int LO, int HI>
constexpr bool in_range(int v) { return LO <= v && v <= HI; }
template <int... V>
constexpr bool one_of(int v) { return ((v == V) || ...); }
constexpr auto flag = in_range<0, 1>;

struct OptionRow {
    const char *key;
    int Options::*member;               // where the value goes, or null with a setter of the row's own
    bool (*accept)(int);
    const char *refusal;                // null: "<key> must be 0 or 1"
    void (*store)(Options &, int) = nullptr;
};

inline const OptionRow kOptionTable[] = {
    {"brick_xcd", &Options::brick_xcd, flag, nullptr},
    {"brick_byte_limit", nullptr, in_range<0, INT_MAX>, "brick_byte_limit must be 0 (the default 2^31) or 1..2^31-1",
     [](Options &o, int v) { o.brick_limit = v == 0 ? (int64_t)1 << 31 : v; }},
    {"den_group", &Options::den_group_opt, [](int v) { return v >= 0 && v <= 64 && (v & (v - 1)) == 0; },
     "den_group must be 0 (automatic) or a power of two up to 64"},
    {"cg_mr_fold", &Options::cg_mr_fold, flag, nullptr},
    {"ho_brick_mfma", &Options::ho_brick_mfma, flag, nullptr},
    {"brick_stagger", &Options::brick_stagger, in_range<-1, 511>, "brick_stagger must be -1 (automatic), 0 (off) or 1..511"},
    {"pa_uniform", &Options::pa_uniform, flag, nullptr},  // the matrix is formed by cdfem_pa_setup; 0 leaves it unused
    {"pa_uniform_diag", &Options::pa_uniform_diag, flag, nullptr},  // the table is built with the Jacobi scale; 0 leaves it unused
    {"ho_uniform", &Options::ho_uniform, flag, nullptr},  // the matrix is formed by cdfem_pa_setup when 1; 0 leaves it unused
    {"ho_uniform_grid", &Options::ho_uniform_grid, in_range<0, INT_MAX>,
     "ho_uniform_grid must be 0 (automatic) or the number of workgroups"},
    {"brick_mfma", &Options::brick_mfma, flag, nullptr},
    {"ho_block_z", &Options::ho_block_z, one_of<2, 4>, "ho_block_z must be 2 or 4"},  // read by cdfem_mesh_set_structured
    {"ho_brick", &Options::ho_brick, flag, nullptr},
    {"mr_overlap", &Options::mr_overlap, flag, nullptr},
    {"brick_mult_pb", &Options::brick_mult_pb, flag, nullptr},
    {"cg_beta_fold", &Options::cg_beta_fold, flag, nullptr},
    {"cg_beta_sum", &Options::cg_beta_sum, flag, nullptr},
    {"cg_den_fold", &Options::cg_den_fold, [](int v) { return v == 0 || (v >= 64 && v <= 16384); },
     "cg_den_fold must be 0 or 64..16384"},
    {"brick_upd_pb", &Options::brick_upd_pb, flag, nullptr},
    {"ho_dfold", &Options::ho_dfold, flag, nullptr},
    {"ho_mfma", &Options::ho_mfma, one_of<0, 1, 3, 8, 9, 15>, "ho_mfma must be 0, 1, 3, 8, 9 or 15"},
    {"cg_xfold", &Options::cg_xfold, flag, nullptr},
    {"cg_fused", &Options::cg_fused, flag, nullptr},
    {"sell_order", &Options::sell_mode, in_range<0, 8>,
     "sell_order must be 0..8 (0 natural, 1 natural + windows, 2 RCM + windows, 3 auto, 4 RCM, 5 geometric, 6 Morton + windows, 7 Morton, 8 Morton LDS windows / auto)"},
    {"gm_poll", &Options::gm_poll, in_range<1, 64>, "gm_poll must be 1..64"},
    {"gm_pb", &Options::gm_pb, flag, nullptr},
    {"pa_affine", &Options::pa_affine, in_range<0, 2>, "pa_affine must be 0, 1 or 2"},  // read by cdfem_pa_setup
    {"pa_geom", &Options::pa_geom, flag, nullptr},  // read by cdfem_pa_setup
    {"ho_geom", &Options::ho_geom, flag, nullptr},  // read by cdfem_pa_setup
    {"spmv_lpr", &Options::spmv_lpr, one_of<0, 1, 2, 4>, "spmv_lpr must be 0 (auto), 1, 2 or 4"},
    {"spmv_lds", &Options::spmv_lds, [](int v) { return v >= -1 && (v <= 0 || (v % 64 == 0 && v <= 65536)); },
     "spmv_lds must be -1 (auto), 0 (off) or rows per window, a multiple of 64 up to 65536"},
    {"sell_window", &Options::sell_window, [](int v) { return v >= 0 && (v == 0 || (v % 64 == 0 && v <= (1 << 20))); },
     "sell_window must be 0 (auto) or a multiple of 64 up to 2^20"},
    {"gm_ept", &Options::gm_ept, one_of<0, 4, 5, 6, 8>, "gm_ept must be 0 (auto), 4, 5, 6 or 8"},
    {"spmv_xcd", &Options::spmv_xcd, flag, nullptr},
    {"spmv_index16", &Options::spmv_index16, flag, nullptr},
    {"profile_mask", nullptr, in_range<INT_MIN, INT_MAX>, "", [](Options &o, int v) { o.prof_mask = (unsigned)v; }},
};

// looks the key up, validates, stores; the refusal's text (cdfem_last_error's), or empty when stored
inline std::string set_option(Options &o, const char *key, int value)
{
    if (!key) return "key is null";
    for (const OptionRow &r : kOptionTable) {
        if (std::strcmp(r.key, key) != 0) continue;
        if (!r.accept(value)) return r.refusal ? std::string(r.refusal) : std::string(key) + " must be 0 or 1";
        if (r.store) r.store(o, value);
        else o.*r.member = value;
        return {};
    }
    return std::string("unknown option ") + key;
}

}  // namespace cdfem
