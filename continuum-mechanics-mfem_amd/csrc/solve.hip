// solve.hip — the operator apply as the solvers see it, the Jacobi scale, and the four host-side Krylov
// drivers behind cdfem_solve: brick CG, generic CG, GMRES(m), BiCGStab.  Host-side orchestration only:
// the drivers queue kernels (vec_kernels.hip, brick_kernels.hip, gmres.hip, bicgstab.hip) and collectives
// and read a few words of device state back at their checks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "cdfem_internal.hpp"
#include "host_util.hpp"
#include "brick_core.hpp"

namespace cdfem {

// (every structured path keys on the mesh: all of them are off while the nonlinear form's matrix-free
// Jacobian is the current operator, nl_jac_current, or an assembled one, fa_ready: the SpMV runs then)
bool use_brick(const cdfem_ctx *c)
{
    return c->structured && !nl_jac_current(c) && !c->fa_ready && brick_supported(c->dim, c->p) && brick_fits(c);
}

// the high-order brick CG (3D p = 3, 4, affine box with constant coefficients: the Kronecker tile core on
// 2^3-element blocks, brick_kernels.hip k_hobrick_cg, then the brick update); on several ranks a z-slab
// of 2^3 blocks (round 6: the plane pack and exchange of the p = 2 brick CG, rank-local den sums)
bool use_hobrick_cg(const cdfem_ctx *c)
{
    return c->ho_brick != 0 && c->structured && !nl_jac_current(c) && c->qlay == 1 && c->hb_nblk > 0 && tile_kron(c) && tile_den_ok(c) &&
           (!multi_rank(c) || (c->part_mode == 1 && c->hb_ez == kHoBrickEdge)) && !c->fa_ready && brick_fits(c);
}
bool use_brick_cg(const cdfem_ctx *c) { return use_brick(c) || use_hobrick_cg(c); }

// ho_uniform: the block CG applies the common element matrix on the matrix cores (k_hobrick_um); the
// matrix is the PA setup's, for the order and kinds it was formed for, on 2 x 2 x 4 blocks of one rank
// (shared with hobrick_um.hip and brick_kernels.hip)
bool ho_uniform_path(const cdfem_ctx *c)
{
    return c->ho_uniform != 0 && (c->kinds == 7 || c->kinds == 5) && !multi_rank(c) && c->hb_ez == 4 && use_hobrick_cg(c);
}
bool ho_uniform_elem(const cdfem_ctx *c)
{
    return c->d_hoelem != nullptr && c->hoelem_p == c->p && c->hoelem_kinds == c->kinds && ho_uniform_path(c);
}

// operator apply into y (device pointers): Ye = A_e x, y = E->L(Ye) [+ constraint]
void op_apply(cdfem_ctx *c, const double *x, double *y, bool constrained)
{
    if (c->fa_ready) {  // assembled CSR: A, or the eliminated matrix for the constrained operator
        timed(c, CDFEM_K_APPLY, [&] { HIPCHK(launch_spmv(c, constrained, x, y)); });
        return;
    }
    if (use_brick(c)) {
        timed(c, CDFEM_K_APPLY, [&] { HIPCHK(launch_brick_mult(c, x, y, constrained, 1)); });
        timed(c, CDFEM_K_E2L, [&] { HIPCHK(launch_brick_mult(c, x, y, constrained, 2)); });
        return;
    }
    timed(c, CDFEM_K_APPLY, [&] { HIPCHK(launch_apply(c, x, c->d_Ye, constrained)); });
    timed(c, CDFEM_K_E2L, [&] { HIPCHK(launch_e2l(c, c->d_Ye, x, y, constrained, 0)); });
}

// the operator on the global (all-rank) space, rank-local L-vectors: the local apply, then the
// shared planes summed with the neighbours (MFEM P^T A P on the true dofs, then P), and for the
// constrained operator the essential rows reset to the identity (an essential dof on a shared
// plane was set by both ranks, so the sum doubled it)
void op_apply_global(cdfem_ctx *c, const double *x, double *y, bool constrained)
{
    op_apply(c, x, y, constrained);
    if (!multi_rank(c)) return;
    interface_sum(c, y);
    if (constrained) HIPCHK(launch_set_ess(c, y, x));
}

namespace {

// n <= 8 host doubles summed over the ranks in place: staged through d_small, read back, stream idle after
void host_allreduce(cdfem_ctx *c, double *h, int n)
{
    if (!c->d_small) c->d_small.alloc(8);
    HIPCHK(hipMemcpyAsync(c->d_small, h, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    comm_allreduce(c, c->d_small, n);
    HIPCHK(hipMemcpyAsync(h, c->d_small, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

using Clock = std::chrono::steady_clock;

const double *ones_vector(cdfem_ctx *c)
{
    if (!c->d_ones) {
        const std::vector<double> one(c->nl, 1.0);
        upload(c, c->d_ones, one);
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return c->d_ones;
}

// the Jacobi scale in the order the running solve uses (mesh order, or the permuted SpMV order)
const double *solver_dinv(cdfem_ctx *c)
{
    ensure_dinv(c);
    if (!c->perm_space) return c->d_dinv;
    if (!c->d_dinv_p) c->d_dinv_p.alloc(c->nl);
    HIPCHK(launch_perm(c, true, c->d_dinv, c->d_dinv_p));
    return c->d_dinv_p;
}

// cg_mr_fold all-reduces partial vectors, so every rank must take it and hold as many partials as the
// others: the apply's (one per brick) and the update's (cg_den_fold_grid).  Decided by every rank of a
// multi-rank solve from the all-reduced eligibility flags and the sums of the counts and of their
// squares (equal on every rank, so every rank takes the same branch): the fold runs iff every rank is
// eligible and the counts' variance is zero.  The 5-double all-reduce runs on EVERY multi-rank brick CG
// entry, whatever the rank's local state (a cached decision let one rank skip the
// collective after an option change that left its own key unchanged while another rank's key moved).
bool mr_fold_agreed(cdfem_ctx *c)
{
    const double ok = cg_mr_fold(c) ? 1.0 : 0.0, nb = den_parts(c), ng = cg_den_fold_grid(c);
    double h[5] = {ok, nb, nb * nb, ng, ng * ng};
    host_allreduce(c, h, 5);
    const double n = c->nranks;
    return h[0] == n && h[2] * n == h[1] * h[1] && h[4] * n == h[3] * h[3];
}

// ---- what the drivers share ----------------------------------------------------------------------

// a solve's opening: the stream idle, then the clock
Clock::time_point solve_begin(cdfem_ctx *c)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    return Clock::now();
}

// and its closing: the clock, the profile's events, the result (fill reads the final state), x out
template <typename Fill>
void solve_end(cdfem_ctx *c, Clock::time_point t0, cdfem_solver_result &res, const double *x, double *dX, Fill &&fill)
{
    const auto t1 = Clock::now();
    prof_collect(c);
    fill();
    res.seconds = std::chrono::duration<double>(t1 - t0).count();
    HIPCHK(hipMemcpyAsync(dX, x, c->nl * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
}

// MFEM CGSolver's start: r = B - A 0, z = M^{-1} r, d = z, nom = (r, z) and the state (all-reduced on several ranks)
void cg_start(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *x, double *r, double *z, double *d,
              const double *dinv)
{
    if (multi_rank(c)) {
        HIPCHK(launch_cg_init_nofin(c, dB, x, r, z, d, dinv));
        comm_allreduce(c, c->d_state->red + 2, 1);
        HIPCHK(launch_init_step(c, p.rel_tol, p.abs_tol, p.max_iter));
    } else {
        HIPCHK(launch_cg_init(c, dB, x, r, z, d, dinv, p.rel_tol, p.abs_tol, p.max_iter));
    }
}

// a CG check: the device state read back; true when the solve is over
bool cg_check(cdfem_ctx *c, int launched, int max_iter)
{
    HIPCHK(hipMemcpyAsync(c->h_state, c->d_state, sizeof(KrylovState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return c->h_state->done || launched >= max_iter;
}

// the result of a CG solve from the state of its last check
void cg_result(const cdfem_ctx *c, cdfem_solver_result &res)
{
    const KrylovState &s = *c->h_state;
    res.converged = s.converged;
    res.iterations = s.final_iter;
    res.initial_norm = std::sqrt(std::fabs(s.nom0));
    res.final_norm = (s.final_iter == 0) ? std::sqrt(std::fabs(s.nom0)) : std::sqrt(std::fabs(s.betanom));
}

// leading dimension of a block of vectors, padded to 32 doubles: every vector starts on a 256-byte
// boundary, so a wave's 512-byte load of v_i covers 4 cache lines, not 5 (odd n)
int64_t padded_ld(int64_t n) { return (n + 31) / 32 * 32; }

// the preconditioner of GMRES and BiCGStab: Jacobi's scale in the solve's order, or null (none, and
// ILU(0), which is factored here and applied by ilu_apply)
const double *resolve_pc(cdfem_ctx *c, const cdfem_solver_params &p)
{
    if (p.pc == CDFEM_PC_JACOBI) return solver_dinv(c);
    if (p.pc == CDFEM_PC_ILU) {
        if (!c->fa_ready) throw UnsupportedError("ILU(0) needs an assembled operator (cdfem_fa_setup)");
        if (multi_rank(c) && c->part_mode != 2)
            throw UnsupportedError("block-Jacobi ILU(0) needs a general partition (cdfem_set_shared)");
        ilu_setup(c);
    }
    return nullptr;
}

// one rank on the structured patch-buffer Mult (set_option "gm_pb"): the solver's kernels form A_c u from
// the patch buffer itself, so phase 1 of the Mult alone runs (the patch buffer is the result)
bool patch_mult(const cdfem_ctx *c, bool ilu)
{
    return c->gm_pb != 0 && !ilu && !multi_rank(c) && use_brick(c) && brick_mult_pb_on(c);
}
void patch_mult_phase1(cdfem_ctx *c, const double *u, double *w)
{
    timed(c, CDFEM_K_APPLY, [&] { HIPCHK(launch_brick_mult(c, u, w, true, 1)); });
}

// brick-path CG (MFEM CGSolver arithmetic): per iteration k_brick_cg (direction + apply + den
// partials) -> den finalizer -> k_cg_update_faces (q assembly + x, r update + betanom partials) ->
// betanom finalizer.  The search direction alternates between two buffers.
void solve_cg_brick(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *dX, cdfem_solver_result &res)
{
    double *x = c->d_w[2], *r = c->d_w[3], *q = c->d_w[4];
    if (!c->d_dalt) c->d_dalt.alloc(c->nl);
    const int nbrick = brick_count(c);
    if (!c->d_face) {  // (p = 3, 4: the blocks' patch buffer, first use)
        const int S = brick_patch_side(c), SZ = brick_patch_side_z(c);
        c->d_face.alloc((size_t)nbrick * S * S * SZ);
    }
    // the apply's den partials in two stages (a block per 1/256 of them, then one block) when the one
    // block finalizer would sum too many: the p = 3, 4 blocks, and one rank past the den fold's bound
    const int ndp = den_parts(c);  // the den partials the folds sum (grouped past the bounds: den_group)
    const bool two_stage = c->p >= 3 || (!multi_rank(c) && ndp > kDenFoldMaxParts);
    if (two_stage && !c->d_hbpart) c->d_hbpart.alloc(nbrick);
    c->den_out = two_stage && c->p <= 2 ? c->d_hbpart : nullptr;
    struct DenOutReset {
        cdfem_ctx *c;
        ~DenOutReset() { c->den_out = nullptr; c->den_grp = 1; }
    } den_out_reset{c};
    double *dprev = c->d_w[5], *dcur = c->d_dalt;
    const double *dinv;
    if (p.pc == CDFEM_PC_JACOBI) {
        ensure_dinv(c);
        dinv = c->d_dinv;
    } else {
        dinv = ones_vector(c);
    }
    const int check = p.check_every > 0 ? p.check_every : 16;
    const bool mr = multi_rank(c);
    double *red = c->d_state->red;  // device scalars awaiting the all-reduce
    const auto t0 = solve_begin(c);
    cg_start(c, p, dB, x, r, q, dprev, dinv);
    // slab partition: the shared planes' partial sums come from the first and last brick layers
    // only, so those layers run first on a side stream, whose pack + exchange then overlap the
    // interior layers on the main stream.  Same kernels, same sums: bitwise equal
    // to the one-launch form.  Profiling keeps the one-launch form (one timed apply kernel).
    const bool overlap = mr && c->mr_overlap && !c->profile && c->p <= 2 && c->nbz >= 3;
    if (overlap && !c->stream2) {
        HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        for (auto &e : c->ov_ev) e.create(false);
    }
    // x-fold (set_option "cg_xfold", default): every apply after the first advances x by the previous
    // iteration's alpha d (the update kernel then streams neither x nor d); k_cg_xflush adds the
    // last update's term after the loop when the update logic stopped the solve
    const bool xfold = c->cg_xfold != 0 && pa_af(c) == 2;  // Kronecker kernel only
    double *const dbuf0 = dcur, *const dbuf1 = dprev;  // apply j writes d_j into dbuf[(j - 1) & 1]
    // betanom fold (cg_beta_fold): apply j > 0 takes the betanom step of update j - 1 (nupd updates so
    // far); the loop always ends with an apply, so every update's step runs
    // several ranks (cg_mr_fold): the den and betanom partial vectors are all-reduced and both folds
    // run as on one rank; the per-iteration kernels are then the one-rank pair plus the plane pack
    const bool mrfold = mr && mr_fold_agreed(c);
    const bool bfold = mr ? mrfold : cg_beta_fold_ok(c);
    // grouped den partials: taken when a fold sums them (several ranks: the fold; one rank: the den fold)
    const int grp = (mr ? mrfold : (!two_stage && cg_den_fold_on(c))) ? den_group(c) : 1;
    if (grp > 1 && c->d_gsum.size() < (size_t)ndp) {
        c->d_gsum.alloc(ndp);
        c->d_gcnt.alloc(ndp);
        HIPCHK(hipMemsetAsync(c->d_gcnt, 0, (size_t)ndp * sizeof(uint32_t), c->stream));
    }
    c->den_grp = grp;
    // cg_beta_sum: the betanom sum and the update's arrival counter (zeroed once: the last arriver resets it)
    if (!mr && bfold && !c->d_bsum) {
        c->d_bsum.alloc(2);
        HIPCHK(hipMemsetAsync(c->d_bsum, 0, 2 * sizeof(double), c->stream));
    }
    double *const dparts = grp > 1 ? c->d_gsum : c->d_part;  // what the mr fold all-reduces (ndp of them)
    int nupd = 0;
    int napply = 0;
    auto mr_den = [&] {  // several ranks, after the exchange: the apply's den over the ranks (overlap: p <= 2)
        if (mrfold) {
            comm_allreduce(c, dparts, ndp);  // the den partials: the update sums them
        } else {
            if (c->p >= 3) HIPCHK(launch_den_local_from_partials(c, c->d_hbpart, nbrick));  // (one per block)
            else HIPCHK(launch_fin_sum(c, nbrick, 0));
            comm_allreduce(c, red + 0, 1);  // den step: folded into the update kernel
        }
    };
    auto apply = [&] {
        double *xf = (xfold && napply > 0) ? x : nullptr;
        ++napply;
        if (overlap) {
            HIPCHK(hipEventRecord(c->ov_ev[0], c->stream));
            HIPCHK(hipStreamWaitEvent(c->stream2, c->ov_ev[0], 0));
            // boundary layers on the side stream, interior layers queued on the main stream
            // before the (possibly host-blocking) exchange is issued
            HIPCHK(launch_brick_cg2_split(c, r, dinv, dprev, dcur, q, c->stream2, xf, bfold ? nupd : -1));
            HIPCHK(launch_pack_qplanes(c, q, c->stream2));
            comm_exchange(c, c->d_if[0], c->d_if[1], c->d_if[2], c->d_if[3], c->Lx * c->Ly, c->stream2);
            HIPCHK(hipEventRecord(c->ov_ev[1], c->stream2));
            HIPCHK(hipStreamWaitEvent(c->stream, c->ov_ev[1], 0));
            mr_den();
            return;
        }
        timed(c, CDFEM_K_APPLY, [&] { HIPCHK(launch_brick_cg2(c, r, dinv, dprev, dcur, q, xf, bfold ? nupd : -1)); });
        prof_mark(c, CDFEM_K_E2L, true);
        if (mr) {
            // neighbours' partial sums of q on the shared planes (added by the update kernel)
            HIPCHK(launch_pack_qplanes(c, q));
            comm_exchange(c, c->d_if[0], c->d_if[1], c->d_if[2], c->d_if[3], c->Lx * c->Ly);
            mr_den();
        } else if (two_stage) {
            HIPCHK(launch_den_from_partials(c, c->d_hbpart, nbrick));  // (one partial per brick / block)
        } else if (!cg_den_fold_on(c)) {
            HIPCHK(launch_den_fin(c, nbrick));  // (cg_den_fold: the update kernel takes the den step)
        }
        prof_mark(c, CDFEM_K_E2L, false);
    };
    apply();
    int launched = 0;
    do {
        for (int k = 0; k < check && launched < p.max_iter; ++k, ++launched) {
            timed(c, CDFEM_K_UPDATE, [&] {
                HIPCHK(launch_cg_update_faces(c, x, r, q, dcur, dinv, mr && c->zlo_shared ? c->d_if[1] : nullptr,
                                              mr && c->zhi_shared ? c->d_if[3] : nullptr, mr && !mrfold, xfold));
                if (mrfold) {
                    comm_allreduce(c, c->d_part + c->nblk, cg_den_fold_grid(c));  // the next apply sums them
                } else if (mr) {
                    comm_allreduce(c, red + 1, 1);
                    HIPCHK(launch_update_step(c));
                }
            });
            ++nupd;
            std::swap(dprev, dcur);
            apply();
        }
    } while (!cg_check(c, launched, p.max_iter));
    if (xfold) {
        HIPCHK(launch_cg_xflush(c, x, dbuf0, dbuf1));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    solve_end(c, t0, res, x, dX, [&] { cg_result(c, res); });
}

// MFEM CGSolver on the constrained operator, device-resident
void solve_cg(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *dX, cdfem_solver_result &res)
{
    double *x = c->d_w[2], *r = c->d_w[3], *z = c->d_w[4], *d = c->d_w[5];
    const double *dinv = p.pc == CDFEM_PC_JACOBI ? solver_dinv(c) : nullptr;
    const int check = p.check_every > 0 ? p.check_every : 16;
    const bool mr = multi_rank(c);
    double *red = c->d_state->red;  // device scalars awaiting the all-reduce (multi-rank)
    // high order on a structured box, one rank: den from the apply's E-vector, E->L fused into the
    // update (ho_kernels.hip k_apply3d_tile<DEN>, vec_kernels.hip k_e2l_box<UPD>)
    const bool fused = !mr && !c->fa_ready && !nl_jac_current(c) && c->cg_fused && tile_den_ok(c) && e2l_box_ok(c) &&
                       c->nl < ((int64_t)1 << 31);  // the flat update's fast division is exact below 2^31
    if (fused && !c->d_tpart) c->d_tpart.alloc(tile_den_blocks(c, true));
    // direction fold (ho_dfold): apply j forms d_j = z + beta d_{j-1} into the other direction buffer
    const bool dfold = fused && tile_dfold_ok(c);
    if (dfold && !c->d_dalt) c->d_dalt.alloc(c->nl);
    double *dprev = d, *dcur = dfold ? c->d_dalt : d;
    const auto t0 = solve_begin(c);
    cg_start(c, p, dB, x, r, z, d, dinv);
    // z = A d ; den = (d, z) and the MFEM den step
    auto apply = [&] {
        prof_mark(c, CDFEM_K_APPLY, true);
        if (fused) {  // Ye = A_c d and den; q stays an E-vector until the update
            if (dfold) HIPCHK(launch_apply_den_dfold(c, z, dprev, dcur, c->d_Ye, c->d_state, c->d_tpart));
            else HIPCHK(launch_apply_den(c, d, c->d_Ye, c->d_state, c->d_tpart));
            prof_mark(c, CDFEM_K_APPLY, false);
            timed(c, CDFEM_K_E2L, [&] { HIPCHK(launch_den_from_partials(c, c->d_tpart, tile_den_blocks(c))); });
            return;
        }
        if (c->fa_ready && !mr) {
            HIPCHK(launch_spmv_cg(c, d, z));
            prof_mark(c, CDFEM_K_APPLY, false);
            return;
        }
        if (c->fa_ready) HIPCHK(launch_spmv(c, true, d, z));
        else HIPCHK(launch_apply_st(c, d, c->d_Ye, true, c->d_state));
        prof_mark(c, CDFEM_K_APPLY, false);
        prof_mark(c, CDFEM_K_E2L, true);
        if (mr) {  // rank partition: interface sums, essential rows reset, owned den all-reduced
            if (!c->fa_ready) HIPCHK(launch_e2l(c, c->d_Ye, d, z, true, 0));
            interface_sum(c, z);
            HIPCHK(launch_set_ess(c, z, d));
            HIPCHK(launch_den_local(c, d, z));
            comm_allreduce(c, red + 0, 1);
            HIPCHK(launch_den_step(c));
        } else {
            HIPCHK(launch_e2l(c, c->d_Ye, d, z, true, 1));
        }
        prof_mark(c, CDFEM_K_E2L, false);
    };
    apply();
    int launched = 0;
    do {
        for (int k = 0; k < check && launched < p.max_iter; ++k, ++launched) {
            timed(c, CDFEM_K_UPDATE, [&] {
                if (fused) HIPCHK(launch_e2l_cg_update(c, c->d_Ye, dcur, x, r, z, dinv));
                else HIPCHK(launch_cg_update(c, x, r, z, d, dinv));
                if (mr) {
                    comm_allreduce(c, red + 1, 1);
                    HIPCHK(launch_update_step(c));
                }
            });
            if (dfold) std::swap(dprev, dcur);
            else timed(c, CDFEM_K_DIRECTION, [&] { HIPCHK(launch_cg_direction(c, z, d)); });
            apply();
        }
    } while (!cg_check(c, launched, p.max_iter));
    solve_end(c, t0, res, x, dX, [&] { cg_result(c, res); });
}

// PETSc KSPGMRES(m) + left Jacobi on the constrained operator (gmres.hip).  One host sync per
// restart cycle plus the lag-one poll (LagPoll, krylov_host.hpp) inside the cycle: a step queued past
// the end of a cycle costs one wasted operator apply (its GMRES kernels exit at entry).
void solve_gmres(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *dX, cdfem_solver_result &res)
{
    const int m = p.restart > 0 ? p.restart : 30;
    if (m > kGmMaxRestart) throw ArgError("restart > 64");
    const int64_t n = c->nl;
    const int64_t ldv = padded_ld(n);
    const int nb = gmres_blocks(n);
    if (c->d_gm.size() < (size_t)(m + 1) * ldv) {  // (the first solve of this mesh, or a longer restart)
        c->d_gm.alloc((size_t)(m + 1) * ldv);
        c->d_gm_part.alloc((size_t)(m + 1) * nb);
    }
    // poll slots: 0 for the cycle start / end, 1 + j for inner step j (each step its own slot, so a
    // host check reads exactly the state of the step it waited for: ranks decide alike)
    krylov_state_alloc(c->d_gmst, c->h_gmpoll, kGmMaxRestart + 1, c->gm_ev);
    const bool ilu = p.pc == CDFEM_PC_ILU;
    const double *dinv = resolve_pc(c, p);
    double *x = c->d_w[2], *w = c->d_w[4], *V = c->d_gm, *part = c->d_gm_part;
    GmresState *st = c->d_gmst;
    GmresHead *poll = c->h_gmpoll;
    // the step's last scalar kernel has written poll[slot] (post_head); the event marks its completion
    // for the host.  (Measured alternatives, profiles/r03/ab_c2_gmres_poll.txt: spinning on a stamp in
    // pinned memory, 392.2 / 392.0 against 392.3 us per C2 step; polling every 2 / 4 / 30 steps, 390.3 /
    // 388.4 / 388.0 against 391.5: the host wait is not on the critical path.)
    auto post = [&](int ev) { HIPCHK(hipEventRecord(c->gm_ev[ev], c->stream)); };
    auto sync = [&](int ev) { HIPCHK(hipEventSynchronize(c->gm_ev[ev])); };
    auto wait = [&](int slot) -> const GmresHead & {  // the synchronous checks of slot 0, on event 0
        sync(slot);
        return poll[slot];
    };
    // pass 1 forms A_c v_j from the patch buffer itself
    const bool gpb = patch_mult(c, ilu);
    // gm_poll k (default 4): an event and a host check every k inner steps (and at a cycle's last step)
    // instead of every step: each event costs the GPU ~5 us before the next Mult (rocprofv3 trace gaps,
    // profiles/r06/ab_gmres_poll/; C2 step 181.3-182.8 -> 178.1-178.2 us at k = 4).  Every step's last
    // scalar kernel posts the state head into its own slot poll[1 + j]; the Mult runs at most 2k - 1 times
    // past the end of a converged cycle (LagPoll).
    const int pk = std::max(1, c->gm_poll);
    LagPoll lag(post, sync);
    const auto t0 = solve_begin(c);
    HIPCHK(hipMemsetAsync(x, 0, n * sizeof(double), c->stream));
    HIPCHK(launch_gm_init(c, st, m, p.max_iter));
    for (bool first = true;; first = false) {
        // v0 = M^{-1}(b - A x); x = 0 on the first cycle, so A x is skipped there
        if (!first) op_apply_global(c, x, w, true);
        if (ilu) {  // v0 = (LU)^{-1} (b - A x): the residual into w, the sweeps into ilu.z
            if (first) HIPCHK(hipMemcpyAsync(w, dB, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            else HIPCHK(launch_axpby(c, 1.0, dB, -1.0, w));
            HIPCHK(ilu_apply(c));
            HIPCHK(launch_gm_residual(c, c->ilu.z, nullptr, nullptr, V, part, st, first, p.rel_tol, p.abs_tol,
                                      &poll[0]));
        } else {
            HIPCHK(launch_gm_residual(c, dB, first ? nullptr : w, dinv, V, part, st, first, p.rel_tol, p.abs_tol,
                                      &poll[0]));
        }
        post(0);
        if (wait(0).done) break;
        for (int j = 0; j < m; ++j) {
            const double *Vj = V + (int64_t)j * ldv;
            GmPatchSrc src{};
            if (gpb) {  // the structured Mult's patch buffer, summed per row by pass 1 (gm_pb)
                patch_mult_phase1(c, Vj, w);
                src = gm_patch_src(c, Vj);
            } else {
                op_apply_global(c, Vj, w, true);
                if (ilu) HIPCHK(ilu_apply(c));  // w <- (LU)^{-1} A v_j, in ilu.z
            }
            timed(c, CDFEM_K_ORTH, [&] {
                HIPCHK(launch_gm_orth(c, ilu ? c->ilu.z : w, dinv, V, ldv, part, st, m, &poll[1 + j], gpb ? &src : nullptr));
            });
            if (j != m - 1 && (j + 1) % pk != 0) continue;
            const int prev = lag.post(j);
            if (prev >= 0 && poll[1 + prev].cycle_done) break;  // exactly that step's state
        }
        lag.reset();
        timed(c, CDFEM_K_UPDATE, [&] { HIPCHK(launch_gm_update(c, x, V, ldv, st, &poll[0])); });
        post(0);
        if (wait(0).done) break;
    }
    solve_end(c, t0, res, x, dX, [&] {
        GmresState fin{};
        HIPCHK(hipMemcpy(&fin, st, sizeof(GmresState), hipMemcpyDeviceToHost));
        res.converged = fin.converged;
        res.iterations = fin.its;
        res.initial_norm = fin.res0;
        res.final_norm = fin.res;
    });
}

// PETSc KSPBCGS + left preconditioning on the constrained operator (bicgstab.hip): seven L-vectors, two
// operator applies per iteration, no orthogonalisation.  The host queues iterations without waiting
// for the device: every check_every-th iteration's last scalar kernel posts the head of the state into
// the pinned slot (i / check_every) % kBcgsSlots, a function of the iteration number alone and so the
// same on every rank, and the host reads a posted iteration's slot one check later (LagPoll,
// krylov_host.hpp).  A slot is rewritten kBcgsSlots checks later, after the host has read it.  At most
// 2 check_every - 1 iterations, that is 2 (2 check_every - 1) operator applies, run past the stop (and
// never more than max_iter iterations in all).
void solve_bicgstab(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *dX, cdfem_solver_result &res)
{
    const int64_t n = c->nl;
    const int64_t ldv = padded_ld(n);
    const int nb = bcgs_blocks(n);
    if (!c->d_bcgs) {  // (the first BiCGStab solve of this mesh)
        c->d_bcgs.alloc((size_t)6 * ldv);
        c->d_bcgs_part.alloc((size_t)3 * nb);
    }
    krylov_state_alloc(c->d_bcst, c->h_bcpoll, kBcgsSlots + 1, c->bc_ev);
    const bool ilu = p.pc == CDFEM_PC_ILU;
    const double *dinv = resolve_pc(c, p);
    double *x = c->d_bcgs, *r = x + ldv, *rh = r + ldv, *pv = rh + ldv, *v = pv + ldv, *t = v + ldv;
    double *w = c->d_w[4], *part = c->d_bcgs_part;  // w: the apply's output (and ilu_apply's input)
    BcgsState *st = c->d_bcst;
    BcgsHead *poll = c->h_bcpoll;
    // k_bcgs_v / k_bcgs_t form A_c u from the patch buffer itself
    const bool gpb = patch_mult(c, ilu);
    c->bcgs_src = gpb ? kBrick * c->p + 1 : 0;
    c->bcgs_diag = dinv ? 1 : 0;
    const int ce = p.check_every > 0 ? p.check_every : 16;
    // w = A_c u, or phase 1 of the structured Mult alone; then M^{-1}
    auto mult = [&](const double *u) -> const double * {
        if (gpb) {
            patch_mult_phase1(c, u, w);
            return w;
        }
        op_apply_global(c, u, w, true);
        if (!ilu) return w;
        HIPCHK(ilu_apply(c));  // ilu.z = (LU)^{-1} w
        return c->ilu.z;
    };
    const auto t0 = solve_begin(c);
    HIPCHK(hipMemsetAsync(x, 0, n * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(pv, 0, n * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(v, 0, n * sizeof(double), c->stream));
    const double *b0 = dB;
    if (ilu) {  // r = (LU)^{-1} B
        HIPCHK(hipMemcpyAsync(w, dB, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(ilu_apply(c));
        b0 = c->ilu.z;
    }
    timed(c, CDFEM_K_UPDATE, [&] {
        HIPCHK(launch_bcgs_init(c, b0, dinv, r, rh, part, st, p.rel_tol, p.abs_tol, p.max_iter, &poll[kBcgsSlots]));
    });
    auto post = [&](int ev) { HIPCHK(hipEventRecord(c->bc_ev[ev], c->stream)); };
    auto sync = [&](int ev) { HIPCHK(hipEventSynchronize(c->bc_ev[ev])); };
    post(0);  // the start slot, synchronously
    sync(0);
    LagPoll lag(post, sync);
    for (int i = 0; i < p.max_iter && !poll[kBcgsSlots].done; ++i) {
        const bool polled = (i + 1) % ce == 0;
        const int slot = (i / ce) % kBcgsSlots;
        timed(c, CDFEM_K_UPDATE, [&] { HIPCHK(launch_bcgs_p(c, r, pv, v, st)); });
        const double *ap = mult(pv);
        const GmPatchSrc srcp = gpb ? gm_patch_src(c, pv) : GmPatchSrc{};
        timed(c, CDFEM_K_UPDATE, [&] { HIPCHK(launch_bcgs_v(c, ap, dinv, rh, v, r, part, st, gpb ? &srcp : nullptr)); });
        const double *as = mult(r);
        const GmPatchSrc srcs = gpb ? gm_patch_src(c, r) : GmPatchSrc{};
        timed(c, CDFEM_K_UPDATE, [&] {
            HIPCHK(launch_bcgs_t(c, as, dinv, x, pv, r, t, rh, part, st, polled ? &poll[slot] : nullptr,
                                 gpb ? &srcs : nullptr));
        });
        if (!polled) continue;
        const int prev = lag.post(slot);
        if (prev >= 0 && poll[prev].done) break;  // exactly that iteration's state
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    solve_end(c, t0, res, x, dX, [&] {
        BcgsState fin{};
        HIPCHK(hipMemcpy(&fin, st, sizeof(BcgsState), hipMemcpyDeviceToHost));
        res.converged = fin.converged;
        res.iterations = fin.its;
        res.initial_norm = fin.res0;
        res.final_norm = fin.dp;
        if (fin.breakdown)
            c->err = fin.breakdown == kBcgsBreakRho  ? "BiCGStab breakdown: rho = (r, rh) is zero"
                     : fin.breakdown == kBcgsBreakD1 ? "BiCGStab breakdown: (v, rh) is zero"
                                                     : "BiCGStab breakdown: (t, t) is zero with a nonzero s";
    });
}

}  // namespace

void ensure_dinv(cdfem_ctx *c)
{
    if (c->dinv_ready) return;
    double *diag = c->d_w[7];
    if (c->fa_ready) {
        HIPCHK(launch_csr_diag(c, diag));
    } else {
        HIPCHK(launch_diag_elem(c, c->d_Ye));
        HIPCHK(launch_e2l(c, c->d_Ye, nullptr, diag, false, 0));
    }
    interface_sum(c, diag);  // shared planes: the full diagonal (both ranks' elements)
    HIPCHK(launch_dinv(c, diag, c->d_dinv));
    // pa_uniform_diag: the class table of a uniform p = 2 box, checked against the vector on the device.
    // Several ranks keep it only if every rank's check passed (each picks a class's entry at the same
    // (x, y) of a shared plane, so the ranks' copies of the plane stay bitwise equal).
    if (nl_jac_current(c) || c->fa_ready) c->d_udiag.reset();  // (J(u)'s diagonal has no classes; the CSR's feeds no brick kernel)
    else HIPCHK(setup_uniform_diag(c));
    if (multi_rank(c)) {
        double all = c->d_udiag ? 1.0 : 0.0;
        host_allreduce(c, &all, 1);
        if (all != (double)c->nranks) c->d_udiag.reset();
    }
    c->dinv_ready = true;
}

void solve(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *dX, cdfem_solver_result &res)
{
    if (p.method == CDFEM_CG) {
        if (use_brick_cg(c)) solve_cg_brick(c, p, dB, dX, res);
        else solve_cg(c, p, dB, dX, res);
    } else if (p.method == CDFEM_BICGSTAB) {
        solve_bicgstab(c, p, dB, dX, res);
    } else {
        solve_gmres(c, p, dB, dX, res);
    }
}

void check_solver_params(const cdfem_solver_params &p)
{
    if (p.max_iter < 0) throw ArgError("max_iter < 0");
    if (p.pc != CDFEM_PC_NONE && p.pc != CDFEM_PC_JACOBI && p.pc != CDFEM_PC_ILU) throw ArgError("unknown preconditioner");
    if (p.pc == CDFEM_PC_ILU && p.method == CDFEM_CG)
        throw UnsupportedError("ILU(0) preconditions GMRES (a nonsymmetric preconditioner for CG)");
    if (p.method != CDFEM_CG && p.method != CDFEM_GMRES && p.method != CDFEM_BICGSTAB) throw ArgError("unknown method");
}

void solve_mesh_order(cdfem_ctx *c, const cdfem_solver_params &p, const double *dB, double *dX, cdfem_solver_result &res)
{
    // permuted SpMV layout (sell_plan.cpp): the Krylov iteration runs in the SpMV's order, B in
    // and X out are permuted once per solve.  ILU(0) factors the matrix in mesh order (PETSc's
    // natural ordering), so it keeps the mesh order and permutes around each apply instead.
    const bool pspace = c->fa_ready && c->d_rperm && !multi_rank(c) && p.pc != CDFEM_PC_ILU;
    struct SpaceGuard {
        cdfem_ctx *c;
        ~SpaceGuard() { c->perm_space = false; }
    } guard{c};
    const double *dBs = dB;
    double *dXs = dX;
    if (pspace) {
        HIPCHK(launch_perm(c, true, dB, c->d_pv[0]));
        dBs = c->d_pv[0];
        dXs = c->d_pv[1];
        c->perm_space = true;
    }
    solve(c, p, dBs, dXs, res);
    if (pspace) {
        c->perm_space = false;
        HIPCHK(launch_perm(c, false, dXs, dX));
    }
}

}  // namespace cdfem
