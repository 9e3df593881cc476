// ho_kernels.hip — high-order (3D p = 3, 4) partial-assembly apply: one Q1 x Q1 THREAD TILE PER
// ELEMENT, quadrature planes (z) in registers.
//
// BASELINE config C3 (128^3 hex, H1 order 4: D1 = 5 dofs and Q1 = 6 Gauss points per direction,
// 125 dofs and 216 points per element).  Thread (tx, ty) of an element's 6 x 6 tile owns the
// column of points (qx = tx, qy = ty, qz = 0..Q1-1):
//   gather   X[dz][dy][dx]                    threads (dx, dy), 5 loads each        -> LDS
//   stage x  BX, GX [dz][dy][qx]              threads (qx, dy)                      -> LDS
//   stage y  bb, bg, gb [dz]                  threads (qx, qy), kept in registers
//   stage z, quadrature-point operator and stage z^T, fused per plane qz, all in registers:
//            u, ux, uy, uz = B_z/G_z contractions of the column;
//            v0 = C.grad u + M u, (vx, vy, vz) = D grad u with this thread's qdata;
//            w0[dz] += B[qz][dz] v0 + G[qz][dz] vz, wx[dz] += B vx, wy[dz] += B vy.
//            The z tables are uniform across the block (kernel arguments, compile-time indices:
//            scalar registers), so this stage reads no LDS at all.
//   stage y^T ZB, ZG [dz][dy][qx]             threads (qx, dy)                      -> LDS
//   stage x^T Y[dz][dy][dx] -> E-vector       threads (dx, dy); element-major (summed by k_e2l) or,
//            on structured boxes, the pencil layout of ho_eidx (summed by k_e2l_box)
// Four barriers per element.  The previous wave-per-element kernel kept every intermediate in
// LDS and read the 1D tables from LDS in every FMA (~270 KB of LDS traffic per element, which
// bounded it at 9.4 ms / 0.54 of HBM); this tile reads ~55 KB.
//
// qdata layout (cdfem_ctx::qlay = 1): qd_ho_index() — per element and plane qz one block of
// nc x Q1^2 doubles with components paired ([pair][qxy][2]), so every thread reads its point's
// components with 16-byte loads and an element's tile reads 576 contiguous bytes per pair.  The
// whole element's qdata (Q1 planes) is issued at kernel entry, in flight behind the gather and the
// x / y stages.  Streaming (non-temporal) loads keep the L-vector in L2 for the gathers.
//
// Geometry mode (set_option "ho_geom", off by default; MF & 32): on a hex mesh the affine forms do not take,
// with constant coefficients, qd is the element-major geometry array (pa_core.hpp HoGeomLayout: 24 doubles
// per element) and every thread forms its points' operator from the trilinear map, plane by plane, as
// elem_apply3d<..., GEO> does: no qdata stream, 96-154 VGPRs, three waves per SIMD.
//
// MFMA (set_option "ho_mfma", off by default): the four LDS stages also exist as block-wide GEMMs
// on v_mfma_f64_16x16x4_f64 (block_mfma below).  On gfx950 the f64 MFMA rate is ~1.2x the f64
// vector FMA rate and these contractions fill at most half of a 16x16x4 tile; the kernel is
// bounded by the qdata stream (8 * 10 * 216 bytes per element against ~20 k FMA), so one stage on
// the matrix cores measures even and more stages measure slower.
#include <hip/hip_runtime.h>

#include "cdfem_internal.hpp"
#include "dispatch.hpp"
#include "pa_core.hpp"
#include "reduce.hpp"

namespace cdfem {

// structured-box geometry of the lattice gather / pencil E-vector (LAT = true)
struct TileGeo {
    HoLayout ho;
    uint32_t Lx, Ly, nz;
    const uint8_t *ess;
};

// DEN (CG mode, structured box, constrained): the block also publishes its share of
// den = (d, A_c d) from the E-vector it writes, sum_e sum_l d~[map(e,l)] Ye[e,l] (d~ = d with the
// essential entries zeroed), plus d_i^2 for each essential DoF i counted once, in the element
// that owns it (the highest element index along each axis).  That is exactly (d, q) with q the
// constrained L-vector, so the E->L sum no longer has to precede the den step and can be fused
// into the CG update (k_e2l_box<UPD>).
// (v4d_t and block_mfma: pa_core.hpp)

// The tile apply's LDS stages as block GEMMs (MF bit k = stage on the matrix cores):
//   bit 0  stage x    [BX | GX](e dz dy, qx)      = X(e dz dy, dx) . [B | G]^T(dx, qx)
//   bit 1  stage y    [bb | gb](e dz qx, qy)      = BX(e dz qx, dy) . [B | G]^T(dy, qy),
//                      bg(e dz qx, qy)           = GX(e dz qx, dy) . B^T(dy, qy)
//   bit 2  stage y^T  [ZB | ZG](e dz qx, dy)      = [W0 | Wy | Wx](e dz qx, qy) . [[B 0]; [G 0]; [0 B]](qy, dy)
//   bit 3  stage x^T  Y(e dz dy, dx)              = [ZB | ZG](e dz dy, qx) . [B; G](qx, dx)
// Each writes LDS; the VALU z stage and quadrature-point operator stay per thread.

template <int D1, int Q1, unsigned K, bool CON, bool LAT, bool DEN, int MF>
__global__ void __launch_bounds__(256)
k_apply3d_tile(const int32_t *__restrict__ map, const double *__restrict__ x, const double *__restrict__ qd,
               double *__restrict__ Ye, const Tab<D1, Q1> T, const int ne, const TileGeo geo,
               const KrylovState *__restrict__ st, double *__restrict__ part)
{
    static_assert(!DEN || (CON && LAT), "den partials need the constrained lattice path");
    static_assert((MF & 32) == 0 || MF == 32, "the geometry form excludes the affine factors and the MFMA stages");
    if (st != nullptr && st->done) return;
    using L = QLayout<K, 3>;
    constexpr bool GEO = (MF & 32) != 0;
    constexpr int NC = L::nc, NP = NC / 2, QQ = Q1 * Q1, ND = D1 * D1 * D1;
    constexpr int PS = qd_ho_plane(NC, Q1);  // doubles per (element, plane) block
    constexpr int EPB = 256 / QQ;            // elements per block
    constexpr int SA = 3 * D1 * QQ;          // X, then W0 / Wx / Wy [dz][qy][qx]
    constexpr int SB = 2 * D1 * D1 * Q1;     // BX / GX, then ZB / ZG [dz][dy][qx]
    static_assert(SA >= ND, "LDS buffer sizes");
    __shared__ double sBt[Q1 * D1], sGt[Q1 * D1], sW[Q1];
    __shared__ double bufA[EPB][SA];
    __shared__ double bufB[EPB][SB];

    const int le = threadIdx.x / QQ, t = threadIdx.x - le * QQ;
    const int tx = t % Q1, ty = t / Q1;
    const int e = blockIdx.x * EPB + le;
    const bool valid = le < EPB && e < ne;
    if (threadIdx.x < Q1 * D1) {
        const int q = threadIdx.x / D1, d = threadIdx.x % D1;
        sBt[threadIdx.x] = T.B[q][d];
        sGt[threadIdx.x] = T.G[q][d];
        if (d == 0) sW[q] = T.w[q];
    }
    double *A = bufA[le < EPB ? le : 0], *Bf = bufB[le < EPB ? le : 0];

    // gather X[dz][dy][dx] (threads dx = tx, dy = ty) into registers FIRST: vmcnt retires in
    // issue order, so loads issued before the qdata stream can be waited for without waiting for
    // the stream.  All loads are unconditional (clamped indices), so gather, stream and the
    // first wait share one basic block and the wait covers only the gather.  Structured boxes
    // (LAT) address x by lattice arithmetic (no map, no dependent load); generic meshes read the
    // element-major map.
    const bool gthr = valid && tx < D1 && ty < D1;
    const int ec = valid ? e : ne - 1;
    const int gx = tx < D1 ? tx : D1 - 1, gy = ty < D1 ? ty : D1 - 1;
    uint32_t ex = 0, ey = 0, ez = 0;
    double xr[D1];
    int32_t m[D1];  // LAT: ess flag; map path: map entry
    size_t g0 = 0, sz = 0;
    if constexpr (LAT) {
        const uint32_t r = fdiv((uint32_t)ec, geo.ho.fnx);
        ex = (uint32_t)ec - r * geo.ho.nx;
        ez = fdiv(r, geo.ho.fny);
        ey = r - ez * geo.ho.ny;
        constexpr int P = D1 - 1;
        g0 = (size_t)(ex * P + gx) + (size_t)geo.Lx * ((ey * P + gy) + (size_t)geo.Ly * (ez * P));
        sz = (size_t)geo.Lx * geo.Ly;
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            xr[dz] = x[g0 + dz * sz];
            m[dz] = CON ? geo.ess[g0 + dz * sz] : 0;
        }
    } else {
        const int32_t *me = map + (size_t)ec * ND + gy * D1 + gx;
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) m[dz] = me[dz * D1 * D1];
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) xr[dz] = x[m[dz] < 0 ? -m[dz] - 1 : m[dz]];
    }
    // this thread's qdata, all planes, in flight from here on (the scheduling barrier keeps the
    // gather loads ahead of the stream in issue order)
    __builtin_amdgcn_sched_barrier(0);
    double qv[GEO ? 1 : Q1][GEO ? 1 : NC];
    // GEO (ho_geom): qd holds GeomLayout's header and then [e][HoGeomLayout::kNC], the coefficients a1..a7 of
    // the element's trilinear map (every thread of a tile reads the same 11 x 16 bytes), and this thread's
    // reference coordinates xi = point[tx], eta = point[ty].  A clamped thread reads element ne - 1, a real
    // element (det J != 0); its results are discarded.
    double ga[GEO ? 22 : 1], gxi = 0.0, geta = 0.0;
    if constexpr (GEO) {
        const v2d_t *ge = reinterpret_cast<const v2d_t *>(qd + GeomLayout::kHdr + (size_t)ec * HoGeomLayout::kNC);
#pragma unroll
        for (int p = 0; p < 11; ++p) {
            const v2d_t w = ge[p];
            ga[2 * p] = w.x;
            ga[2 * p + 1] = w.y;
        }
        gxi = qd[GeomLayout::hPts + tx];
        geta = qd[GeomLayout::hPts + ty];
    } else if constexpr ((MF & 16) != 0) {
        // affine factors (pa_affine): qd holds g[e][NC]; the point data W_q g_k with W_q = (w_x w_y) w_z,
        // the product the setup stores (k_setup_qdata), formed after the table barrier below
#pragma unroll
        for (int k = 0; k < NC; ++k) qv[0][k] = qd[(size_t)ec * NC + k];
    } else {
        const double *qe = qd + (size_t)ec * Q1 * PS;
#pragma unroll
        for (int qz = 0; qz < Q1; ++qz) {
            const double *qp = qe + qz * PS;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const v2d_t w = __builtin_nontemporal_load(reinterpret_cast<const v2d_t *>(qp + p * 2 * QQ) + t);
                qv[qz][2 * p] = w.x;
                qv[qz][2 * p + 1] = w.y;
            }
            if constexpr (NC & 1) qv[qz][NC - 1] = __builtin_nontemporal_load(qp + 2 * NP * QQ + t);
        }
    }
    // unconditional store (a conditional one lets the compiler sink the gather loads behind the
    // stream): threads outside the gather write into the unused tail of bufA
    static_assert(ND + QQ * D1 <= SA, "junk slots");
#pragma unroll
    for (int dz = 0; dz < D1; ++dz) {
        const bool zero = CON && (LAT ? m[dz] != 0 : m[dz] < 0);
        A[gthr ? (dz * D1 + ty) * D1 + tx : ND + t * D1 + dz] = zero ? 0.0 : xr[dz];
    }
    __syncthreads();
    if constexpr ((MF & 16) != 0) {
        double g[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) g[k] = qv[0][k];
        const double wxy = sW[tx < Q1 ? tx : 0] * sW[ty < Q1 ? ty : 0];
#pragma unroll
        for (int qz = 0; qz < Q1; ++qz) {
            const double W = wxy * T.w[qz];
#pragma unroll
            for (int k = 0; k < NC; ++k) qv[qz][k] = W * g[k];
        }
    }
    // GEO: the parts of J that are fixed along this thread's column of points (pa_core.hpp elem_apply3d,
    // GEO: x = a0 + a1 xi + a2 eta + a3 zeta + a4 xi eta + a5 xi zeta + a6 eta zeta + a7 xi eta zeta):
    //     dx/dxi   = (a1 + eta a4) + zeta (a5 + eta a7)         gp0 + zeta gp1
    //     dx/deta  = (a2 + xi a4) + zeta (a6 + xi a7)           gq0 + zeta gq1
    //     dx/dzeta = (a3 + eta a6) + xi (a5 + eta a7)           gc2, constant along the column
    // and w_x w_y; 15 doubles against the stream's Q1 * NC
    double gp0[3] = {}, gp1[3] = {}, gq0[3] = {}, gq1[3] = {}, gc2[3] = {}, gwxy = 0.0;
    if constexpr (GEO) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gp0[i] = ga[0 + i] + geta * ga[9 + i];
            gp1[i] = ga[12 + i] + geta * ga[18 + i];
            gq0[i] = ga[3 + i] + gxi * ga[9 + i];
            gq1[i] = ga[15 + i] + gxi * ga[18 + i];
            gc2[i] = (ga[6 + i] + geta * ga[15 + i]) + gxi * gp1[i];
        }
        gwxy = sW[tx] * sW[ty];
    }
    // stage x: threads (qx = tx, dy = ty), or the matrix cores (MF & 1)
    constexpr int DD = D1 * D1, DQ = D1 * Q1;
    if constexpr ((MF & 1) != 0) {
        static_assert(2 * Q1 <= 16, "one tile of output columns");
        block_mfma<EPB * DD, (D1 + 3) / 4>(
            [&](int row, int k) { return k < D1 ? bufA[row / DD][(row % DD) * D1 + k] : 0.0; },
            [&](int k, int col) {
                return k >= D1 ? 0.0 : col < Q1 ? sBt[col * D1 + k] : col < 2 * Q1 ? sGt[(col - Q1) * D1 + k] : 0.0;
            },
            [&](int row, int col, double v) {
                if (col < 2 * Q1)
                    bufB[row / DD][(col < Q1 ? 0 : DD * Q1) + (row % DD) * Q1 + (col < Q1 ? col : col - Q1)] = v;
            });
    } else if (valid && ty < D1) {
        double b[D1], g[D1];
#pragma unroll
        for (int dx = 0; dx < D1; ++dx) {
            b[dx] = sBt[tx * D1 + dx];
            g[dx] = sGt[tx * D1 + dx];
        }
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            double bx = 0.0, gx = 0.0;
#pragma unroll
            for (int dx = 0; dx < D1; ++dx) {
                const double xv = A[(dz * D1 + ty) * D1 + dx];
                bx += b[dx] * xv;
                gx += g[dx] * xv;
            }
            Bf[(dz * D1 + ty) * Q1 + tx] = bx;
            Bf[D1 * D1 * Q1 + (dz * D1 + ty) * Q1 + tx] = gx;
        }
    }
    __syncthreads();
    // stage y: threads (qx = tx, qy = ty), column over dz in registers
    double bb[D1], bg[D1], gb[D1];
    if constexpr ((MF & 2) != 0) {
        // rows (e, dz, qx); the results land in bufA (X is dead) at the slots this thread's z
        // stage later overwrites with W0 / Wx / Wy, so reading them back needs no extra barrier
        auto ain = [&](int off) {
            return [&, off](int row, int k) {
                if (k >= D1) return 0.0;
                const int e = row / DQ, r = row % DQ, dz = r / Q1, qx = r % Q1;
                return bufB[e][off + (dz * D1 + k) * Q1 + qx];
            };
        };
        block_mfma<EPB * DQ, (D1 + 3) / 4>(
            ain(0),
            [&](int k, int col) {
                return k >= D1 ? 0.0 : col < Q1 ? sBt[col * D1 + k] : col < 2 * Q1 ? sGt[(col - Q1) * D1 + k] : 0.0;
            },
            [&](int row, int col, double v) {
                const int e = row / DQ, r = row % DQ, dz = r / Q1, qx = r % Q1;
                if (col < Q1) bufA[e][dz * QQ + col * Q1 + qx] = v;                        // bb
                else if (col < 2 * Q1) bufA[e][(2 * D1 + dz) * QQ + (col - Q1) * Q1 + qx] = v;  // gb
            });
        block_mfma<EPB * DQ, (D1 + 3) / 4>(
            ain(DD * Q1), [&](int k, int col) { return k < D1 && col < Q1 ? sBt[col * D1 + k] : 0.0; },
            [&](int row, int col, double v) {
                const int e = row / DQ, r = row % DQ, dz = r / Q1, qx = r % Q1;
                if (col < Q1) bufA[e][(D1 + dz) * QQ + col * Q1 + qx] = v;  // bg
            });
        __syncthreads();
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            bb[dz] = A[dz * QQ + t];
            bg[dz] = A[(D1 + dz) * QQ + t];
            gb[dz] = A[(2 * D1 + dz) * QQ + t];
        }
    } else {
        double by[D1], gy[D1];
#pragma unroll
        for (int dy = 0; dy < D1; ++dy) {
            by[dy] = sBt[ty * D1 + dy];
            gy[dy] = sGt[ty * D1 + dy];
        }
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int dy = 0; dy < D1; ++dy) {
                const int i = (dz * D1 + dy) * Q1 + tx;
                const double bxv = Bf[i], gxv = Bf[D1 * D1 * Q1 + i];
                s0 += by[dy] * bxv;
                s1 += by[dy] * gxv;
                s2 += gy[dy] * bxv;
            }
            bb[dz] = s0;
            bg[dz] = s1;
            gb[dz] = s2;
        }
    }
    // stage z + quadrature-point operator + stage z^T, plane by plane in registers
    double w0[D1], wx[D1], wy[D1];
#pragma unroll
    for (int dz = 0; dz < D1; ++dz) w0[dz] = wx[dz] = wy[dz] = 0.0;
#pragma unroll
    for (int qz = 0; qz < Q1; ++qz) {
        // GEO: the planes one after another.  A plane's geometry depends on nothing else in the loop, and
        // left alone the compiler forms adj J and det J of all Q1 planes ahead of it and defers the
        // accumulations (Q1 * 13 doubles live at once; 201-240 VGPRs, or spills under a bound).  The empty
        // asm statements keep their order: zeta and the column's inputs pass through one at the head of
        // the plane, the accumulators through one each at its end.
        double zeta = 0.0;
        if constexpr (GEO) {
            zeta = qd[GeomLayout::hPts + qz];
            if constexpr (L::kD || L::kC) asm volatile("" : "+v"(zeta), "+v"(bb[0]), "+v"(bg[0]), "+v"(gb[0]));
            else asm volatile("" : "+v"(zeta), "+v"(bb[0]));
        }
        double u = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            const double bz = T.B[qz][dz], gz = T.G[qz][dz];
            u += bz * bb[dz];
            uz += gz * bb[dz];
            ux += bz * bg[dz];
            uy += bz * gb[dz];
        }
        double v0 = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
        if constexpr (GEO) {
            // the point operator in its factors, as elem_apply3d<..., GEO>: tg = adj(J)^T grad_ref u, then
            // D grad_ref u = (W kappa / det J) adj(J) tg, C . grad_ref u = W (alpha c) . tg, M u = (W s det J) u
            const double W = gwxy * T.w[qz];
            double c0[3], c1[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                c0[i] = gp0[i] + zeta * gp1[i];
                c1[i] = gq0[i] + zeta * gq1[i];
            }
            double Aj[3][3];  // adj(J): rows c1 x c2, c2 x c0, c0 x c1
            cross3(c1, gc2, Aj[0]);
            const double det = c0[0] * Aj[0][0] + c0[1] * Aj[0][1] + c0[2] * Aj[0][2];
            double tg[3] = {0.0, 0.0, 0.0};
            if constexpr (L::kD || L::kC) {
                cross3(gc2, c0, Aj[1]);
                cross3(c0, c1, Aj[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) tg[k] = Aj[0][k] * ux + Aj[1][k] * uy + Aj[2][k] * uz;
            }
            if constexpr (L::kD) {
                const double sd = W * qd[GeomLayout::hKappa] * rcp_nr(det);
                const double s0 = sd * tg[0], s1 = sd * tg[1], s2 = sd * tg[2];
                vx = Aj[0][0] * s0 + Aj[0][1] * s1 + Aj[0][2] * s2;
                vy = Aj[1][0] * s0 + Aj[1][1] * s1 + Aj[1][2] * s2;
                vz = Aj[2][0] * s0 + Aj[2][1] * s1 + Aj[2][2] * s2;
            }
            if constexpr (L::kC)
                v0 = W * (qd[GeomLayout::hConv] * tg[0] + qd[GeomLayout::hConv + 1] * tg[1] +
                          qd[GeomLayout::hConv + 2] * tg[2]);
            if constexpr (L::kM) v0 += (W * qd[GeomLayout::hMass] * det) * u;
        } else {
            if constexpr (L::kD) {
                const double d00 = qv[qz][0], d01 = qv[qz][1], d02 = qv[qz][2];
                const double d11 = qv[qz][3], d12 = qv[qz][4], d22 = qv[qz][5];
                vx = d00 * ux + d01 * uy + d02 * uz;
                vy = d01 * ux + d11 * uy + d12 * uz;
                vz = d02 * ux + d12 * uy + d22 * uz;
            }
            if constexpr (L::kC) v0 += qv[qz][L::oC] * ux + qv[qz][L::oC + 1] * uy + qv[qz][L::oC + 2] * uz;
            if constexpr (L::kM) v0 += qv[qz][L::oM] * u;
        }
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            const double bz = T.B[qz][dz], gz = T.G[qz][dz];
            w0[dz] += bz * v0 + gz * vz;
            wx[dz] += bz * vx;
            wy[dz] += bz * vy;
        }
        if constexpr (GEO) {
#pragma unroll
            for (int dz = 0; dz < D1; ++dz) {
                asm volatile("" : "+v"(w0[dz]));
                if constexpr (L::kD) asm volatile("" : "+v"(wx[dz]), "+v"(wy[dz]));
            }
        }
    }
    // X (bufA) was last read in stage x, before the previous barrier
    if (le < EPB) {
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            A[dz * QQ + t] = w0[dz];
            A[(D1 + dz) * QQ + t] = wx[dz];
            A[(2 * D1 + dz) * QQ + t] = wy[dz];
        }
    }
    __syncthreads();
    // stage y^T: threads (qx = tx, dy = ty); BX / GX (bufB) were last read in stage y
    if constexpr ((MF & 4) != 0) {
        // rows (e, dz, qx), k = (W0 | Wy | Wx, qy) padded to 4 KS, cols (ZB | ZG, dy)
        constexpr int KY = 3 * Q1;
        block_mfma<EPB * DQ, (KY + 3) / 4>(
            [&](int row, int k) {
                if (k >= KY) return 0.0;
                const int e = row / DQ, r = row % DQ, dz = r / Q1, qx = r % Q1;
                const int which = k / Q1, qy = k % Q1;  // 0: W0, 1: Wy, 2: Wx
                const int blk = which == 0 ? 0 : which == 1 ? 2 : 1;
                return bufA[e][(blk * D1 + dz) * QQ + qy * Q1 + qx];
            },
            [&](int k, int col) {
                if (k >= KY || col >= 2 * D1) return 0.0;
                const int which = k / Q1, qy = k % Q1;
                if (col < D1) return which == 0 ? sBt[qy * D1 + col] : which == 1 ? sGt[qy * D1 + col] : 0.0;
                return which == 2 ? sBt[qy * D1 + col - D1] : 0.0;
            },
            [&](int row, int col, double v) {
                if (col >= 2 * D1) return;
                const int e = row / DQ, r = row % DQ, dz = r / Q1, qx = r % Q1;
                const int dy = col < D1 ? col : col - D1;
                bufB[e][(col < D1 ? 0 : DD * Q1) + (dz * D1 + dy) * Q1 + qx] = v;
            });
    } else if (valid && ty < D1) {
        double cb[Q1], cg[Q1];
#pragma unroll
        for (int qy = 0; qy < Q1; ++qy) {
            cb[qy] = sBt[qy * D1 + ty];
            cg[qy] = sGt[qy * D1 + ty];
        }
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            double zb = 0.0, zg = 0.0;
#pragma unroll
            for (int qy = 0; qy < Q1; ++qy) {
                const int j = dz * QQ + qy * Q1 + tx;
                zb += cb[qy] * A[j] + cg[qy] * A[2 * D1 * QQ + j];
                zg += cb[qy] * A[D1 * QQ + j];
            }
            Bf[(dz * D1 + ty) * Q1 + tx] = zb;
            Bf[D1 * D1 * Q1 + (dz * D1 + ty) * Q1 + tx] = zg;
        }
    }
    __syncthreads();
    // stage x^T -> E-vector: threads (dx = tx, dy = ty)
    if constexpr ((MF & 8) != 0) {
        // rows (e, dz, dy), k = (ZB | ZG, qx), cols dx; Y into bufA (W0 / Wx / Wy are dead)
        block_mfma<EPB * DD, (2 * Q1 + 3) / 4>(
            [&](int row, int k) {
                if (k >= 2 * Q1) return 0.0;
                const int e = row / DD, r = row % DD;
                return bufB[e][(k < Q1 ? 0 : DD * Q1) + r * Q1 + (k < Q1 ? k : k - Q1)];
            },
            [&](int k, int col) {
                return k >= 2 * Q1 || col >= D1 ? 0.0 : k < Q1 ? sBt[k * D1 + col] : sGt[(k - Q1) * D1 + col];
            },
            [&](int row, int col, double v) {
                if (col < D1) bufA[row / DD][(row % DD) * D1 + col] = v;
            });
        __syncthreads();
    }
    double dacc = 0.0;
    if (valid && tx < D1 && ty < D1) {
        double cb[Q1], cg[Q1];
#pragma unroll
        for (int qx = 0; qx < Q1; ++qx) {
            cb[qx] = sBt[qx * D1 + tx];
            cg[qx] = sGt[qx * D1 + tx];
        }
        double *ye;
        size_t zs;  // stride between dz planes
        if constexpr (LAT) {
            const size_t row = (size_t)geo.ho.nx * D1;
            ye = Ye + (((size_t)ez * D1 * geo.ho.ny + ey) * D1 + ty) * row + (size_t)ex * D1 + tx;
            zs = (size_t)geo.ho.ny * D1 * row;
        } else {
            ye = Ye + (size_t)e * ND + ty * D1 + tx;
            zs = D1 * D1;
        }
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            double y = 0.0;
            if constexpr ((MF & 8) != 0) {
                y = A[(dz * D1 + ty) * D1 + tx];
            } else {
#pragma unroll
                for (int qx = 0; qx < Q1; ++qx) {
                    const int j = (dz * D1 + ty) * Q1 + qx;
                    y += cb[qx] * Bf[j] + cg[qx] * Bf[D1 * D1 * Q1 + j];
                }
            }
            __builtin_nontemporal_store(y, &ye[dz * zs]);
            if constexpr (DEN) {
                constexpr int P = D1 - 1;
                const bool own = (tx < P || ex == geo.ho.nx - 1) && (ty < P || ey == geo.ho.ny - 1) &&
                                 (dz < P || ez == geo.nz - 1);
                dacc += m[dz] != 0 ? (own ? xr[dz] * xr[dz] : 0.0) : xr[dz] * y;
            }
        }
    }
    if constexpr (DEN) {
        __shared__ double shd[256 / 64];
        store_partial(block_sum(dacc, shd), part);
    }
}

// Kronecker-form tile apply (pa_affine 2: affine mesh, constant coefficients, ho_mfma 0).  The
// element operator is sum_t g_t Fz (x) Fy (x) Fx with the rule's 1D matrices (pa_core.hpp
// kron_xrow / kron_y / kron_z), so no stage runs over the Q1 quadrature points: one D1 x D1 thread
// tile per element (25 threads at p = 4, 10 elements per 256-thread block; 16 at p = 3):
//   gather   X[dz][dy][dx]                       threads (dx, dy), D1 loads each     -> LDS
//   x + y    plane jz, output column ix          threads (ix, jz): the five x-applied rows of the
//            plane (kron_xrow on this thread's rows of M, K, C, Ct, loaded from a 100-double device
//            table, ktab: ix is a thread index, so these are the only run-time-indexed constants), then for every
//            output row iy the four z groups P[grp][jz][iy][ix] (kron_y, compile-time tables)   -> LDS
//   z        output (ix, iy), all iz             threads (ix, iy): kron_z over the planes jz, then
//            the E-vector store (and the den partials) exactly as k_apply3d_tile
// Two barriers per element; 5 KB of LDS per element at p = 4, three blocks per CU.
// DF (fused CG, set_option "ho_dfold"): x is z = M^-1 r; the gather also reads d_old and forms the
// direction d = z + beta d_old (k_cg_direction's formula) in registers, and each dof's one owner
// element (the DEN ownership rule) writes it to d_new, so the direction pass disappears.
template <int D1, int Q1, unsigned K, bool CON, bool LAT, bool DEN, bool DF = false>
__global__ void __launch_bounds__(256, 3)
k_apply3d_ktile(const int32_t *__restrict__ map, const double *__restrict__ x, const double *__restrict__ qaff,
                double *__restrict__ Ye, const Tab<D1, Q1> T, const int ne, const TileGeo geo,
                const KrylovState *__restrict__ st, double *__restrict__ part, const double *__restrict__ dold,
                double *__restrict__ dnew, const double *__restrict__ ktab)
{
    static_assert(!DEN || (CON && LAT), "den partials need the constrained lattice path");
    static_assert(!DF || DEN, "the direction fold runs in the fused CG apply");
    if (st != nullptr && st->done) return;
    using L = QLayout<K, 3>;
    constexpr int NC = L::nc, DD = D1 * D1, ND = DD * D1;
    constexpr int EPB = 256 / DD;
    __shared__ double sX[EPB][ND];
    __shared__ double sP[EPB][4][ND];  // [grp][jz][iy][ix]

    const int le = threadIdx.x / DD, t = threadIdx.x - le * DD;
    const int a = t % D1, b = t / D1;
    const int e = blockIdx.x * EPB + le;
    const bool inb = le < EPB, valid = inb && e < ne;
    const int ec = valid ? e : ne - 1;
    // this thread's x-stage rows (ix = a), in flight with the gather
    double Mr[D1], Kr[D1], Cr[D1], Ctr[D1];
#pragma unroll
    for (int j = 0; j < D1; ++j) {
        Mr[j] = ktab[(0 * D1 + a) * D1 + j];
        Kr[j] = ktab[(1 * D1 + a) * D1 + j];
        Cr[j] = ktab[(2 * D1 + a) * D1 + j];
        Ctr[j] = ktab[(3 * D1 + a) * D1 + j];
    }
    // gather X (threads dx = a, dy = b) and the element's factors
    uint32_t ex = 0, ey = 0, ez = 0;
    double xr[D1];
    int32_t m[D1];  // LAT: ess flag; map path: map entry
    if constexpr (LAT) {
        const uint32_t r = fdiv((uint32_t)ec, geo.ho.fnx);
        ex = (uint32_t)ec - r * geo.ho.nx;
        ez = fdiv(r, geo.ho.fny);
        ey = r - ez * geo.ho.ny;
        constexpr int P = D1 - 1;
        const size_t g0 = (size_t)(ex * P + a) + (size_t)geo.Lx * ((ey * P + b) + (size_t)geo.Ly * (ez * P));
        const size_t sz = (size_t)geo.Lx * geo.Ly;
        double ov[D1];
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            xr[dz] = x[g0 + dz * sz];
            if constexpr (DF) ov[dz] = dold[g0 + dz * sz];
            m[dz] = CON ? geo.ess[g0 + dz * sz] : 0;
        }
        if constexpr (DF) {
            const double beta = st->beta;
            const bool ownxy = valid && (a < P || ex == geo.ho.nx - 1) && (b < P || ey == geo.ho.ny - 1);
#pragma unroll
            for (int dz = 0; dz < D1; ++dz) {
                xr[dz] = xr[dz] + beta * ov[dz];
                if (ownxy && (dz < P || ez == geo.nz - 1)) dnew[g0 + dz * sz] = xr[dz];
            }
        }
    } else {
        const int32_t *me = map + (size_t)ec * ND + b * D1 + a;
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) m[dz] = me[dz * DD];
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) xr[dz] = x[m[dz] < 0 ? -m[dz] - 1 : m[dz]];
    }
    double g[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) g[k] = qaff[(size_t)ec * NC + k];
    if (inb) {
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            const bool zero = CON && (LAT ? m[dz] != 0 : m[dz] < 0);
            sX[le][(dz * D1 + b) * D1 + a] = zero ? 0.0 : xr[dz];
        }
    }
    __syncthreads();
    // x + y stages: thread (ix = a, jz = b)
    if (inb) {
        double v[D1][5];
#pragma unroll
        for (int jy = 0; jy < D1; ++jy) {
            const double *xrow = &sX[le][(b * D1 + jy) * D1];
            double mm = 0.0, kk = 0.0, cc = 0.0, ct = 0.0;
#pragma unroll
            for (int jx = 0; jx < D1; ++jx) {
                const double xv = xrow[jx];
                mm += Mr[jx] * xv;
                if constexpr (L::kD) {
                    kk += Kr[jx] * xv;
                    ct += Ctr[jx] * xv;
                }
                if constexpr (L::kD || L::kC) cc += Cr[jx] * xv;
            }
            kron_xcombine<K>(g, mm, kk, cc, ct, v[jy]);
        }
        auto col = [&](int q, int jy) { return v[jy][q]; };
#pragma unroll
        for (int iy = 0; iy < D1; ++iy) {
            double P[4];
            kron_y<D1, Q1, K>(T, g, col, iy, P);
#pragma unroll
            for (int k = 0; k < 4; ++k) sP[le][k][(b * D1 + iy) * D1 + a] = P[k];
        }
    }
    __syncthreads();
    // z stage and the E-vector: thread (ix = dx = a, iy = dy = b)
    double dacc = 0.0;
    if (valid) {
        double Yz[D1];
#pragma unroll
        for (int iz = 0; iz < D1; ++iz) Yz[iz] = 0.0;
#pragma unroll
        for (int jz = 0; jz < D1; ++jz) {
            double P[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) P[k] = sP[le][k][(jz * D1 + b) * D1 + a];
            kron_z<D1, Q1, K>(T, P, jz, Yz);
        }
        double *ye;
        size_t zs;  // stride between dz planes
        if constexpr (LAT) {
            const size_t row = (size_t)geo.ho.nx * D1;
            ye = Ye + (((size_t)ez * D1 * geo.ho.ny + ey) * D1 + b) * row + (size_t)ex * D1 + a;
            zs = (size_t)geo.ho.ny * D1 * row;
        } else {
            ye = Ye + (size_t)e * ND + b * D1 + a;
            zs = DD;
        }
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) {
            __builtin_nontemporal_store(Yz[dz], &ye[dz * zs]);
            if constexpr (DEN) {
                constexpr int P = D1 - 1;
                const bool own = (a < P || ex == geo.ho.nx - 1) && (b < P || ey == geo.ho.ny - 1) &&
                                 (dz < P || ez == geo.nz - 1);
                dacc += m[dz] != 0 ? (own ? xr[dz] * xr[dz] : 0.0) : xr[dz] * Yz[dz];
            }
        }
    }
    if constexpr (DEN) {
        __shared__ double shd[256 / 64];
        store_partial(block_sum(dacc, shd), part);
    }
}

// the x-stage rows of the Kronecker tile kernels (k_apply3d_ktile, brick_kernels.hip k_hobrick_cg):
// canonical entries of make_tab's orbit averages, as tM / tK / tCacc read them, [M | K | C | Ct][i][j]
template <int D1, int Q1>
static hipError_t ktab_build(cdfem_ctx *c, const Tab<D1, Q1> &T)
{
    const int key = c->p * 64 + c->rule_op.q1;
    if (c->ktab_key == key) return hipSuccess;
    // (a rebuild follows a new setup: let any copy still reading h_ktab finish first)
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (es != hipSuccess) return es;
    if (!c->d_ktab) c->d_ktab.alloc(sizeof(c->h_ktab) / sizeof(double));
    for (int i = 0; i < D1; ++i)
        for (int j = 0; j < D1; ++j) {
            const int m = sym_can(D1, i, j), ca = anti_can(D1, i, j), sa = anti_sign(D1, i, j);
            const int cb = anti_can(D1, j, i), sb = anti_sign(D1, j, i);
            c->h_ktab[(0 * D1 + i) * D1 + j] = T.M1[m / D1][m % D1];
            c->h_ktab[(1 * D1 + i) * D1 + j] = T.K1[m / D1][m % D1];
            c->h_ktab[(2 * D1 + i) * D1 + j] = sa == 0 ? 0.0 : sa * T.C1[ca / D1][ca % D1];
            c->h_ktab[(3 * D1 + i) * D1 + j] = sb == 0 ? 0.0 : sb * T.C1[cb / D1][cb % D1];
        }
    const hipError_t e = hipMemcpyAsync(c->d_ktab, c->h_ktab, sizeof(double) * 4 * D1 * D1, hipMemcpyHostToDevice,
                                        c->stream);
    if (e != hipSuccess) return e;
    c->ktab_key = key;
    return hipSuccess;
}

// f(D1, Q1) as constants for p = 3, 4 under the operators' Gauss rule of p + 2 points
template <class F>
static hipError_t dispatch_ho(const cdfem_ctx *c, F &&f)
{
    if (c->rule_op.q1 != c->p + 2) return hipErrorInvalidValue;
    return dispatch_value<3, 4>(c->p, hipErrorInvalidValue, [&](auto P) {
        return f(std::integral_constant<int, P() + 1>{}, std::integral_constant<int, P() + 2>{});
    });
}

hipError_t ho_ktab(cdfem_ctx *c, const double **out)
{
    const hipError_t e = dispatch_ho(c, [&](auto D1, auto Q1) {
        return ktab_build<D1(), Q1()>(c, make_tab<D1(), Q1()>(c->rule_op));
    });
    *out = c->d_ktab;
    return e;
}

template <int D1, int Q1, unsigned K>
static hipError_t ktile_kinds(cdfem_ctx *c, const double *x, double *Ye, bool con, const KrylovState *st,
                              double *den_part, const double *dold = nullptr, double *dnew = nullptr)
{
    const Tab<D1, Q1> T = make_tab<D1, Q1>(c->rule_op);
    constexpr int EPB = 256 / (D1 * D1);
    const dim3 grid((unsigned)((c->ne + EPB - 1) / EPB)), block(256);
    TileGeo geo{};
    geo.ho = ho_layout(c);
    geo.Lx = (uint32_t)c->Lx;
    geo.Ly = (uint32_t)c->Ly;
    geo.nz = c->epencil ? (uint32_t)(c->ne / ((int64_t)geo.ho.nx * geo.ho.ny)) : 0;
    geo.ess = c->d_ess;
    const double *qa = c->d_qaff;
    {
        const hipError_t e = ktab_build<D1, Q1>(c, T);
        if (e != hipSuccess) return e;
    }
    const double *kt = c->d_ktab;
    if (kt == nullptr) return hipErrorInvalidValue;
    // den partials (CG mode) need the constrained apply on the element pencils, the direction fold the den
    const bool den = den_part != nullptr, df = den && dnew != nullptr;
    if (df && !dold) return hipErrorInvalidValue;
    return dispatch_bools(con, c->epencil != 0, den, df, [&](auto CON, auto LAT, auto DEN, auto DF) {
        if constexpr ((DEN() && !(CON() && LAT())) || (DF() && !DEN())) return hipErrorInvalidValue;
        else {
            const auto kern = k_apply3d_ktile<D1, Q1, K, CON(), LAT(), DEN(), DF()>;
            CDFEM_LAUNCH(c, kern, grid, block, 0, c->d_map.get(), x, qa, Ye, T, c->ne, geo, st, den_part,
                         DF() ? dold : nullptr, DF() ? dnew : nullptr, kt);
            return hipGetLastError();
        }
    });
}

// the fused CG apply with the direction fold (ho_dfold): d_new = z + beta d_old, Ye = A_c d_new, den
template <int D1, int Q1>
static hipError_t ktile_dfold(cdfem_ctx *c, const double *z, const double *dold, double *dnew, double *Ye,
                              const KrylovState *st, double *part)
{
    return dispatch_kinds(c->kinds, hipErrorInvalidValue,
                          [&](auto K) { return ktile_kinds<D1, Q1, K()>(c, z, Ye, true, st, part, dold, dnew); });
}

template <int D1, int Q1, unsigned K, int MF>
static hipError_t tile_kinds_mf(cdfem_ctx *c, const double *x, double *Ye, bool con, const KrylovState *st,
                             double *den_part)
{
    const Tab<D1, Q1> T = make_tab<D1, Q1>(c->rule_op);
    constexpr int EPB = 256 / (Q1 * Q1);
    const dim3 grid((unsigned)((c->ne + EPB - 1) / EPB)), block(256);
    TileGeo geo{};
    geo.ho = ho_layout(c);
    geo.Lx = (uint32_t)c->Lx;
    geo.Ly = (uint32_t)c->Ly;
    geo.nz = c->epencil ? (uint32_t)(c->ne / ((int64_t)geo.ho.nx * geo.ho.ny)) : 0;
    geo.ess = c->d_ess;
    const double *qd = (MF & 32) ? c->d_hgeom : (MF & 16) ? c->d_qaff : c->d_qd;
    if (qd == nullptr) return hipErrorInvalidValue;
    // den partials (CG mode) need the constrained apply on the element pencils
    return dispatch_bools(con, c->epencil != 0, den_part != nullptr, [&](auto CON, auto LAT, auto DEN) {
        if constexpr (DEN() && !(CON() && LAT())) return hipErrorInvalidValue;
        else {
            const auto kern = k_apply3d_tile<D1, Q1, K, CON(), LAT(), DEN(), MF>;
            CDFEM_LAUNCH(c, kern, grid, block, 0, c->d_map.get(), x, qd, Ye, T, c->ne, geo, st, den_part);
            return hipGetLastError();
        }
    });
}

template <int D1, int Q1, unsigned K>
static hipError_t tile_kinds(cdfem_ctx *c, const double *x, double *Ye, bool con, const KrylovState *st,
                             double *den_part)
{
    if (tile_kron(c)) return ktile_kinds<D1, Q1, K>(c, x, Ye, con, st, den_part);
    if (tile_affine(c)) {
        // affine factors; on the BASELINE operator (kinds 7) also with the x / x^T stages on the
        // matrix cores (ho_mfma 1, 8, 9: VERDICT r03 item 4, the arithmetic-bound regime)
        // (tile_affine admits no other mask, and none but 0 off kinds 7)
        return dispatch_value<0, 1, 8, 9>(c->ho_mfma, hipErrorInvalidValue, [&](auto M) {
            if constexpr (M() != 0 && K != 7) return hipErrorInvalidValue;
            else return tile_kinds_mf<D1, Q1, K, 16 + M()>(c, x, Ye, con, st, den_part);
        });
    }
    // geometric factors formed in the apply (ho_geom: any hex, constant coefficients, ho_mfma 0)
    if (ho_geom_on(c)) return tile_kinds_mf<D1, Q1, K, 32>(c, x, Ye, con, st, den_part);
    // the stream, with the stages of the mask on the matrix cores; any other mask runs the plain stages
    hipError_t e = hipSuccess;
    const bool masked = dispatch_value<1, 3, 8, 9, 15>(c->ho_mfma, false, [&](auto M) {
        e = tile_kinds_mf<D1, Q1, K, M()>(c, x, Ye, con, st, den_part);
        return true;
    });
    return masked ? e : tile_kinds_mf<D1, Q1, K, 0>(c, x, Ye, con, st, den_part);
}

// the tile apply of x (CG mode, den_part: with the den partials, one per block)
static hipError_t tile_dq(cdfem_ctx *c, const double *x, double *Ye, bool con, const KrylovState *st,
                          double *den_part)
{
    return dispatch_ho(c, [&](auto D1, auto Q1) {
        return dispatch_kinds(c->kinds, hipErrorInvalidValue,
                              [&](auto K) { return tile_kinds<D1(), Q1(), K()>(c, x, Ye, con, st, den_part); });
    });
}

hipError_t launch_apply_wpe(cdfem_ctx *c, const double *x, double *Ye, bool con, const KrylovState *st)
{
    return tile_dq(c, x, Ye, con, st, nullptr);
}

// den partials of the CG-mode tile apply: one per block of the kernel the configuration launches, or
// (most) the quadrature tile's count, which bounds both (D1 < Q1), for the allocation
int tile_den_blocks(const cdfem_ctx *c, bool most)
{
    const int q1 = c->rule_op.q1, t = !most && tile_kron(c) ? c->d1 * c->d1 : q1 * q1;
    return (int)((c->ne + 256 / t - 1) / (256 / t));
}

bool tile_den_ok(const cdfem_ctx *c)
{
    const int q1 = c->rule_op.q1;
    return c->dim == 3 && c->epencil && c->structured && ((c->p == 3 && q1 == 5) || (c->p == 4 && q1 == 6));
}

bool tile_dfold_ok(const cdfem_ctx *c) { return c->ho_dfold != 0 && tile_kron(c) && tile_den_ok(c); }

hipError_t launch_apply_den_dfold(cdfem_ctx *c, const double *z, const double *dold, double *dnew, double *Ye,
                                  const KrylovState *st, double *part)
{
    if (!tile_dfold_ok(c)) return hipErrorInvalidValue;
    return dispatch_ho(c, [&](auto D1, auto Q1) { return ktile_dfold<D1(), Q1()>(c, z, dold, dnew, Ye, st, part); });
}

// CG mode: Ye = A_c d (E-vector) and the den partials (one per block) into part
hipError_t launch_apply_den(cdfem_ctx *c, const double *d, double *Ye, const KrylovState *st, double *part)
{
    return tile_dq(c, d, Ye, true, st, part);
}

}  // namespace cdfem
