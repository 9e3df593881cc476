// bicgstab.hip — BiCGStab with left preconditioning, device-resident.
//
// Semantics: PETSc KSPBCGS with LEFT preconditioning and a zero initial guess on the constrained
// operator A_c; M^{-1} is none, Jacobi or ILU(0) as in gmres.hip.  All dots run over owned entries
// (skip_lo) and are all-reduced on several ranks.
//
//   r = M^{-1} B;  rh = r;  dp = |r|;  res0 = dp;  ttol = max(rtol dp, atol)
//   dp <= ttol (or dp == 0): converged, iterations 0, X = 0;   max_iter == 0: not converged, X = 0
//   rho_old = alpha = omega_old = 1;  p = v = 0;  x = 0
//   for i = 0, 1, ...:
//       rho = (r, rh)                               rho == 0 -> breakdown
//       beta = (rho / rho_old)(alpha / omega_old)
//       p = r + beta (p - omega_old v)
//       v = M^{-1} A_c p;  d1 = (v, rh)             d1 == 0  -> breakdown
//       alpha = rho / d1;  s = r - alpha v
//       t = M^{-1} A_c s;  d1 = (s, t);  d2 = (t, t)
//       d2 == 0:  x += alpha p;  its = i + 1;  dp = 0;  converged if (s, s) == 0, else breakdown;  stop
//       omega = d1 / d2;  x += alpha p + omega s;  r = s - omega t;  dp = |r|
//       rho_old = rho;  omega_old = omega;  its = i + 1
//       dp <= ttol -> converged;  its >= max_iter -> not converged;  dp not finite -> not converged
//
// iterations counts these iterations (two operator applies each), initial_norm = res0, final_norm =
// the last dp.  A breakdown (PETSc KSP_DIVERGED_BREAKDOWN) ends the solve not converged with its
// kind in BcgsState::breakdown.
//
// MI355X layout: seven L-vectors (x, r, rh, p, v, t and the apply's output w; s lives in r) whatever
// the iteration count.  Per iteration, besides the two operator applies:
//   k_bcgs_p      p = r + beta (p - omega v)                                  reads 3 N, writes 1 N
//   k_bcgs_v      v = M^{-1} A_c p, partials of (v, rh)                       reads 3 N, writes 1 N
//   k_bcgs_alpha  d1 summed in fixed order, breakdown test, alpha
//   k_bcgs_s      s = r - alpha v in place over r                             reads 2 N, writes 1 N
//   k_bcgs_t      t = M^{-1} A_c s, partials of (s, t), (t, t), (s, s)        reads 3 N, writes 1 N
//   k_bcgs_omega  the three sums, the d2 == 0 case, omega
//   k_bcgs_x      x += alpha p + omega s, r = s - omega t, partials (r, r), (r, rh)
//                                                                             reads 5 N, writes 2 N
//   k_bcgs_rho    dp, its, the stop tests, the next rho and beta, host poll
// 22 N doubles with Jacobi (19 N without a diagonal; with the patch source the apply's output is
// neither written nor read: the 1-8 patch entries per row are read instead).  (r, rh) for the next
// rho comes from k_bcgs_x, so rho costs no pass of its own.  All reductions: fixed grid, fixed order,
// no floating-point atomics (bitwise reproducible).  Every kernel checks the done flag, so
// iterations the host queued past the stop exit at entry and change nothing.
#include <hip/hip_runtime.h>

#include <cmath>

#include "krylov_core.hpp"

namespace cdfem {

// L-vector entries per thread of the vector kernels (EPT): 4, 5, 6 or 8, chosen per vector size by
// bcgs_ept; a block covers kRedThreads * EPT entries.  The row of A_c u (patch_row), the sums over the
// partials and their all-reduce (summed, launch_summed) and the host poll (post_head): krylov_core.hpp
static int bcgs_nb(int64_t n, int ept) { return (int)((n + (int64_t)kRedThreads * ept - 1) / ((int64_t)kRedThreads * ept)); }
int bcgs_blocks(int64_t n) { return bcgs_nb(n, 4); }  // the most blocks any EPT launches (partials' size)

// ---- r = rh = M^{-1} b, partials of (r, r) ------------------------------------------------------
template <int kBcEPT>
__global__ void __launch_bounds__(kRedThreads)
k_bcgs_init(const double *__restrict__ b, const double *__restrict__ dinv, double *__restrict__ r,
            double *__restrict__ rh, int64_t n, int64_t skip_lo, double *__restrict__ part)
{
    __shared__ double sh[kRedThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * (kRedThreads * kBcEPT) + threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        if (k < n) {
            double v = b[k];
            if (dinv) v *= dinv[k];
            r[k] = v;
            rh[k] = v;
            if (k >= skip_lo) acc += v * v;  // shared plane owned by the rank below
        }
    }
    store_partial(block_sum(acc, sh), part);
}

// ---- dp = |r|, tolerance, the two stops before the first iteration, the first rho and beta -----
__global__ void __launch_bounds__(1024)
k_bcgs_start(const double *__restrict__ part, int nb, BcgsState *__restrict__ st, double rtol, double atol,
             int max_it, int mode, BcgsHead *__restrict__ poll)
{
    __shared__ double sh[1][1024 / 64];
    double sums[1];
    if (!summed(part, nb, st, mode, sh, sums)) return;
    const double sum = sums[0], dp = sqrt(sum);
    st->dp = dp;
    st->res0 = dp;
    st->ttol = fmax(rtol * dp, atol);
    st->max_it = max_it;
    st->its = 0;
    st->breakdown = 0;
    st->half = 0;
    st->converged = 0;
    st->done = 0;
    st->alpha = 1.0;
    st->omega = 1.0;
    if (dp <= st->ttol || dp == 0.0) {
        st->converged = 1;
        st->done = 1;
    } else if (max_it <= 0 || !isfinite(dp)) {
        st->done = 1;
    } else {
        // rh = r: the first rho = (r, rh) is this sum, and with rho_old = alpha = omega_old = 1
        // beta = (rho / rho_old)(alpha / omega_old) = rho (p = v = 0, so the first p is r)
        st->rho = sum;
        st->beta = sum;
    }
    post_head(st, poll);
}

// ---- p = r + beta (p - omega v) ------------------------------------------------------------------
template <int kBcEPT>
__global__ void __launch_bounds__(kRedThreads)
k_bcgs_p(const double *__restrict__ r, double *__restrict__ p, const double *__restrict__ v, int64_t n,
         const BcgsState *__restrict__ st)
{
    if (st->done) return;
    const double beta = st->beta, omega = st->omega;
    const int64_t base = (int64_t)blockIdx.x * (kRedThreads * kBcEPT) + threadIdx.x;
    double rr[kBcEPT], pp[kBcEPT], vv[kBcEPT];
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        const int64_t kc = k < n ? k : n - 1;
        rr[e] = r[kc];
        pp[e] = p[kc];
        vv[e] = v[kc];
    }
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        if (k < n) p[k] = rr[e] + beta * (pp[e] - omega * vv[e]);
    }
}

// ---- v = M^{-1} A_c p, partials of (v, rh) -------------------------------------------------------
template <int S, int kBcEPT>
__global__ void __launch_bounds__(kRedThreads)
k_bcgs_v(const double *__restrict__ w, const double *__restrict__ dinv, const double *__restrict__ rh,
         double *__restrict__ v, int64_t n, int64_t skip_lo, double *__restrict__ part,
         const BcgsState *__restrict__ st, const GmPatchSrc ps)
{
    __shared__ double sh[kRedThreads / 64];
    if (st->done) return;
    const int64_t base = (int64_t)blockIdx.x * (kRedThreads * kBcEPT) + threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        if (k < n) {
            double y = patch_row<S>(w, ps, k);
            if (dinv) y *= dinv[k];
            v[k] = y;
            if (k >= skip_lo) acc += y * rh[k];
        }
    }
    store_partial(block_sum(acc, sh), part);
}

// ---- d1 = (v, rh): breakdown test, alpha = rho / d1 ----------------------------------------------
__global__ void __launch_bounds__(1024)
k_bcgs_alpha(const double *__restrict__ part, int nb, BcgsState *__restrict__ st, int mode)
{
    __shared__ double sh[1][1024 / 64];
    if (st->done) return;  // uniform: every thread reads the same flag before the reduction
    double sums[1];
    if (!summed(part, nb, st, mode, sh, sums)) return;
    const double d1 = sums[0];
    if (d1 == 0.0) {
        st->breakdown = kBcgsBreakD1;
        st->done = 1;
        return;
    }
    st->alpha = st->rho / d1;
}

// ---- s = r - alpha v, in place over r ------------------------------------------------------------
template <int kBcEPT>
__global__ void __launch_bounds__(kRedThreads)
k_bcgs_s(double *__restrict__ r, const double *__restrict__ v, int64_t n, const BcgsState *__restrict__ st)
{
    if (st->done) return;
    const double alpha = st->alpha;
    const int64_t base = (int64_t)blockIdx.x * (kRedThreads * kBcEPT) + threadIdx.x;
    double rr[kBcEPT], vv[kBcEPT];
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        const int64_t kc = k < n ? k : n - 1;
        rr[e] = r[kc];
        vv[e] = v[kc];
    }
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        if (k < n) r[k] = rr[e] - alpha * vv[e];
    }
}

// ---- t = M^{-1} A_c s, partials of (s, t), (t, t), (s, s) ----------------------------------------
template <int S, int kBcEPT>
__global__ void __launch_bounds__(kRedThreads)
k_bcgs_t(const double *__restrict__ w, const double *__restrict__ dinv, const double *__restrict__ s,
         double *__restrict__ t, int64_t n, int64_t skip_lo, double *__restrict__ part, int nb,
         const BcgsState *__restrict__ st, const GmPatchSrc ps)
{
    __shared__ double sh[3][kRedThreads / 64];
    if (st->done) return;
    const int64_t base = (int64_t)blockIdx.x * (kRedThreads * kBcEPT) + threadIdx.x;
    double st_ = 0.0, tt = 0.0, ss = 0.0;
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        if (k < n) {
            double y = patch_row<S>(w, ps, k);
            if (dinv) y *= dinv[k];
            t[k] = y;
            if (k >= skip_lo) {
                const double sk = s[k];
                st_ += sk * y;
                tt += y * y;
                ss += sk * sk;
            }
        }
    }
    const double a = block_sum(st_, sh[0]), b = block_sum(tt, sh[1]), c = block_sum(ss, sh[2]);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a;
        part[(int64_t)nb + blockIdx.x] = b;
        part[2 * (int64_t)nb + blockIdx.x] = c;
    }
}

// ---- d1 = (s, t), d2 = (t, t): omega = d1 / d2, or the d2 == 0 exit (half step: x += alpha p) ----
__global__ void __launch_bounds__(1024)
k_bcgs_omega(const double *__restrict__ part, int nb, BcgsState *__restrict__ st, int mode)
{
    __shared__ double sh[3][1024 / 64];
    if (st->done) return;
    double sums[3];
    if (!summed(part, nb, st, mode, sh, sums)) return;
    const double d1 = sums[0], d2 = sums[1], ss = sums[2];
    if (d2 == 0.0) {  // t = 0: k_bcgs_x adds alpha p alone (omega 0), k_bcgs_rho ends the solve
        st->half = 1;
        st->ss = ss;
        st->omega = 0.0;
        return;
    }
    st->omega = d1 / d2;
}

// ---- x += alpha p + omega s, r = s - omega t, partials of (r, r), (r, rh) ------------------------
template <int kBcEPT>
__global__ void __launch_bounds__(kRedThreads)
k_bcgs_x(double *__restrict__ x, const double *__restrict__ p, double *__restrict__ r,
         const double *__restrict__ t, const double *__restrict__ rh, int64_t n, int64_t skip_lo,
         double *__restrict__ part, int nb, const BcgsState *__restrict__ st)
{
    __shared__ double sh[2][kRedThreads / 64];
    if (st->done) return;
    const double alpha = st->alpha, omega = st->omega;
    const int64_t base = (int64_t)blockIdx.x * (kRedThreads * kBcEPT) + threadIdx.x;
    double xx[kBcEPT], pp[kBcEPT], sv[kBcEPT], tv[kBcEPT], hv[kBcEPT];
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        const int64_t kc = k < n ? k : n - 1;
        xx[e] = x[kc];
        pp[e] = p[kc];
        sv[e] = r[kc];
        tv[e] = t[kc];
        hv[e] = rh[kc];
    }
    double rr = 0.0, rrh = 0.0;
#pragma unroll
    for (int e = 0; e < kBcEPT; ++e) {
        const int64_t k = base + (int64_t)e * kRedThreads;
        if (k < n) {
            x[k] = xx[e] + alpha * pp[e] + omega * sv[e];
            const double rn = sv[e] - omega * tv[e];
            r[k] = rn;
            if (k >= skip_lo) {
                rr += rn * rn;
                rrh += rn * hv[e];
            }
        }
    }
    const double a = block_sum(rr, sh[0]), b = block_sum(rrh, sh[1]);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a;
        part[(int64_t)nb + blockIdx.x] = b;
    }
}

// ---- dp = |r|, its, the stop tests; then the next iteration's rho = (r, rh) and beta --------------
__global__ void __launch_bounds__(1024)
k_bcgs_rho(const double *__restrict__ part, int nb, BcgsState *__restrict__ st, int mode,
           BcgsHead *__restrict__ poll)
{
    __shared__ double sh[2][1024 / 64];
    if (st->done) {
        if (threadIdx.x == 0) post_head(st, poll);
        return;
    }
    double sums[2];
    if (!summed(part, nb, st, mode, sh, sums)) return;
    const double rr = sums[0], rrh = sums[1];
    st->its += 1;
    if (st->half) {  // d2 == 0
        st->dp = 0.0;
        st->converged = st->ss == 0.0 ? 1 : 0;
        if (!st->converged) st->breakdown = kBcgsBreakD2;
        st->done = 1;
    } else {
        const double dp = sqrt(rr);
        st->dp = dp;
        if (dp <= st->ttol) {
            st->converged = 1;
            st->done = 1;
        } else if (st->its >= st->max_it || !isfinite(dp)) {
            st->done = 1;
        } else if (rrh == 0.0) {
            st->breakdown = kBcgsBreakRho;
            st->done = 1;
        } else {
            st->beta = (rrh / st->rho) * (st->alpha / st->omega);
            st->rho = rrh;
        }
    }
    post_head(st, poll);
}

// ---- launchers ---------------------------------------------------------------------------------
// Entries per thread of the vector kernels (pick_ept): the smallest whose grid fits CUs x the resident
// blocks of the widest kernel, k_bcgs_x, at that EPT
static int bcgs_ept(cdfem_ctx *c)
{
    return cached_ept(c->bcgs_ept_auto, c->nl, [](int e) {
        int64_t fit = 0;
        with_ept(e, [&](auto E) { fit = resident_blocks(k_bcgs_x<E()>); });
        return fit;
    });
}

hipError_t launch_bcgs_init(cdfem_ctx *c, const double *b, const double *dinv, double *r, double *rh, double *part,
                            BcgsState *st, double rtol, double atol, int max_it, BcgsHead *poll)
{
    const int ept = bcgs_ept(c), nb = bcgs_nb(c->nl, ept);
    with_ept(ept, [&](auto E) {
        hipLaunchKernelGGL(k_bcgs_init<E()>, dim3(nb), dim3(kRedThreads), 0, c->stream, b, dinv, r, rh, (int64_t)c->nl,
                           (int64_t)c->skip_lo, part);
    });
    launch_summed(c, st->red, 1, poll, [&](int mode, BcgsHead *slot) {
        hipLaunchKernelGGL(k_bcgs_start, dim3(1), dim3(1024), 0, c->stream, part, nb, st, rtol, atol, max_it, mode,
                           slot);
    });
    return hipGetLastError();
}

hipError_t launch_bcgs_p(cdfem_ctx *c, const double *r, double *p, const double *v, BcgsState *st)
{
    with_ept(bcgs_ept(c), [&](auto E) {
        hipLaunchKernelGGL(k_bcgs_p<E()>, dim3(bcgs_nb(c->nl, E())), dim3(kRedThreads), 0, c->stream, r, p, v,
                           (int64_t)c->nl, st);
    });
    return hipGetLastError();
}

// v = M^{-1} A_c p from w (ps null) or the patch buffer, alpha, then s = r - alpha v over r
hipError_t launch_bcgs_v(cdfem_ctx *c, const double *w, const double *dinv, const double *rh, double *v, double *r,
                         double *part, BcgsState *st, const GmPatchSrc *ps)
{
    const int ept = bcgs_ept(c), nb = bcgs_nb(c->nl, ept);
    const int64_t n = c->nl;
    const hipError_t bad = with_patch_src(ps, [&](auto S, const GmPatchSrc &src) {
        with_ept(ept, [&](auto E) {
            hipLaunchKernelGGL((k_bcgs_v<S(), E()>), dim3(nb), dim3(kRedThreads), 0, c->stream, w, dinv, rh, v, n,
                               (int64_t)c->skip_lo, part, st, src);
        });
    });
    if (bad != hipSuccess) return bad;
    launch_summed<BcgsHead>(c, st->red, 1, nullptr, [&](int mode, BcgsHead *) {
        hipLaunchKernelGGL(k_bcgs_alpha, dim3(1), dim3(1024), 0, c->stream, part, nb, st, mode);
    });
    with_ept(ept, [&](auto E) {
        hipLaunchKernelGGL(k_bcgs_s<E()>, dim3(nb), dim3(kRedThreads), 0, c->stream, r, v, n, st);
    });
    return hipGetLastError();
}

// t = M^{-1} A_c s from w (ps null) or the patch buffer, omega, the x and r update, the stop tests
hipError_t launch_bcgs_t(cdfem_ctx *c, const double *w, const double *dinv, double *x, const double *p, double *r,
                         double *t, const double *rh, double *part, BcgsState *st, BcgsHead *poll,
                         const GmPatchSrc *ps)
{
    const int ept = bcgs_ept(c), nb = bcgs_nb(c->nl, ept);
    const int64_t n = c->nl, lo = c->skip_lo;
    const hipError_t bad = with_patch_src(ps, [&](auto S, const GmPatchSrc &src) {
        with_ept(ept, [&](auto E) {
            hipLaunchKernelGGL((k_bcgs_t<S(), E()>), dim3(nb), dim3(kRedThreads), 0, c->stream, w, dinv, r, t, n, lo,
                               part, nb, st, src);
        });
    });
    if (bad != hipSuccess) return bad;
    launch_summed<BcgsHead>(c, st->red, 3, nullptr, [&](int mode, BcgsHead *) {
        hipLaunchKernelGGL(k_bcgs_omega, dim3(1), dim3(1024), 0, c->stream, part, nb, st, mode);
    });
    with_ept(ept, [&](auto E) {
        hipLaunchKernelGGL(k_bcgs_x<E()>, dim3(nb), dim3(kRedThreads), 0, c->stream, x, p, r, t, rh, n, lo, part, nb,
                           st);
    });
    launch_summed(c, st->red, 2, poll, [&](int mode, BcgsHead *slot) {
        hipLaunchKernelGGL(k_bcgs_rho, dim3(1), dim3(1024), 0, c->stream, part, nb, st, mode, slot);
    });
    return hipGetLastError();
}

}  // namespace cdfem
