// krylov_core.hpp — the protocols every device-resident Krylov solver follows, written once (gmres.hip,
// bicgstab.hip): the row of A_c u read from the structured Mult's patch buffer, a sum over the blocks' partials
// that is all-reduced on several ranks, and the state head posted to the host.  What needs no HIP (the
// entries-per-thread rule, the host's side of the poll) is in krylov_host.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "brick_core.hpp"
#include "cdfem_internal.hpp"
#include "dispatch.hpp"
#include "reduce.hpp"

namespace cdfem {

// ---- the patch-buffer row ------------------------------------------------------------------------
// (A_c u)_k from the apply's output w (S == 0), or from the structured Mult's patch buffer: the row's
// 1-8 patch entries in patch_sum8's order, the apply's input on the essential rows (S = 4p + 1)
template <int S>
__device__ __forceinline__ double patch_row(const double *__restrict__ w, const GmPatchSrc &ps, int64_t k)
{
    if constexpr (S == 0) {
        return w[k];
    } else {  // (n < 2^28 on the brick path: brick_fits)
        const uint32_t gid = (uint32_t)k, plane = (uint32_t)(ps.g.Lx * ps.g.Ly);
        const uint32_t gz = fdiv(gid, ps.fdxy), rem = gid - gz * plane, gy = fdiv(rem, ps.fdx);
        const uint32_t gx = rem - gy * (uint32_t)ps.g.Lx;
        const auto bp = brsrc(ps.pb, 8u * (uint32_t)ps.g.nbx * ps.g.nby * ps.g.nbz * (S * S * S));
        double y = patch_sum8<S>(bp, ps.g, (int)gx, (int)gy, (int)gz);
        if (ps.ess[k]) y = ps.x[k];  // A_c: the identity row
        return y;
    }
}

// f(S as a constant, the source by value as the kernels take it): S 0 for w itself (ps null), or the patch
// side, 5 or 9; any other side is refused before anything is launched
template <class F>
hipError_t with_patch_src(const GmPatchSrc *ps, F &&f)
{
    if (ps && ps->S != 5 && ps->S != 9) return hipErrorInvalidValue;
    const GmPatchSrc src = ps ? *ps : GmPatchSrc{};
    (void)dispatch_value<0, 5, 9>(ps ? ps->S : 0, false, [&](auto S) {
        f(S, src);
        return true;
    });
    return hipSuccess;
}

// ---- what pick_ept asks: the blocks (kRedThreads threads) of a vector kernel resident at once, CUs x per CU ----
template <class Kernel>
int64_t resident_blocks(Kernel kernel)
{
    int dev = 0, cus = 0, per = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, kRedThreads, 0);
    return (int64_t)std::max(cus, 1) * std::max(per, 1);
}

// ---- the three-mode sum --------------------------------------------------------------------------
// A one-block scalar kernel sums N partial vectors (part[i * nb .. (i + 1) * nb), each in sum_partials's
// fixed order) and runs the solver's scalar logic on the sums.  On several ranks the sums are all-reduced
// in between, so the kernel runs twice:
//   mode 0  one rank: the block sums, then the logic
//   mode 1  the block sums stored into st->red[0 .. N) (all-reduced next), no logic
//   mode 2  the logic on st->red[0 .. N), the same arithmetic and the same branches on every rank
// summed() fills s[] in every thread (modes 0 and 1: valid in thread 0) and returns true in the one thread
// that runs the logic.  Modes 0 and 1 pass the barrier inside each sum_partials, mode 2 passes none; every
// thread of the block must call it.
template <int N, class State>
__device__ __forceinline__ bool summed(const double *__restrict__ part, int nb, State *__restrict__ st, int mode,
                                       double (&sh)[N][1024 / 64], double (&s)[N])
{
    if (mode == 2) {
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] = st->red[i];
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] = sum_partials(part + (int64_t)i * nb, nb, sh[i]);
    }
    if (threadIdx.x != 0) return false;
    if (mode == 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) st->red[i] = s[i];
        return false;
    }
    return true;
}

// The host half: launch(mode, slot) queues the scalar kernel.  One rank: mode 0.  Several: mode 1, the
// all-reduce of red[0 .. n), mode 2.  The poll slot goes to the one launch that runs the logic.  Every rank
// must issue the same collectives in the same order: a launcher that spells this out differently from
// another rank's deadlocks the all-reduce.
template <class Head, class Launch>
void launch_summed(cdfem_ctx *c, double *red, int n, Head *poll, Launch &&launch)
{
    const bool mr = multi_rank(c);
    launch(mr ? 1 : 0, mr ? nullptr : poll);
    if (mr) {
        comm_allreduce(c, red, n);
        launch(2, poll);
    }
}

// ---- the poll head -------------------------------------------------------------------------------
// Host poll without a copy kernel: the last scalar kernel of every polled step writes the head of the state
// straight into the pinned host slot the host will wait on (hipHostMalloc memory is device-visible; LagPoll).  A D2H
// hipMemcpyAsync of those bytes cost a 4 us blit kernel per GMRES step.  (poll is null on a step that is not polled.)
template <class State, class Head>
__device__ inline void post_head(const State *st, Head *poll)
{
    static_assert(std::is_base_of_v<Head, State>);
    if (!poll) return;
    *poll = *st;
    __threadfence_system();
}

}  // namespace cdfem
