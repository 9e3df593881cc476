// pa_kernels.hip — partial-assembly kernels for H1 tensor elements on gfx950.
//
// Replaces MFEM's DiffusionIntegrator / ConvectionIntegrator / MassIntegrator AssemblePA +
// AddMultPA (called from a.Assemble() and Operator::Mult in linear_convection_diffusion_2D.cpp:
// 335-339, 364-370) with ONE fused operator: per quadrature point
//     v     = M u + C . grad_ref(u)            (mass + convection, test with phi)
//     vgrad = D grad_ref(u)                    (diffusion, test with grad phi)
// where D = W kappa adj(J)adj(J)^T/detJ, C = W alpha adj(J) c, M = W s detJ (qdata, HBM-resident).
//
// Apply kernel mapping (MI355X-first): one THREAD per element, one wavefront per
// 64-element block.  The 1D contractions (sum factorization, x/y/z) run in registers with
// compile-time-unrolled loops, so there is no LDS traffic, no barrier, and every qdata load of a
// wavefront is 512 contiguous bytes.  The element loop is a pure stream over qdata (10 doubles
// per quadrature point at p=2 = 94% of the bytes), which is what bounds the kernel (HBM roofline).
#include <hip/hip_runtime.h>

#include "cdfem_internal.hpp"
#include "dispatch.hpp"
#include "pa_core.hpp"
#include "point_geom.hpp"

namespace cdfem {

// ------------------------------------------------------------------------------------------------
// 3D apply: Ye = A_e x_e for every element (thread per element)
// ------------------------------------------------------------------------------------------------
template <int D1, int Q1, unsigned K, bool CON, int AF>
__global__ void __launch_bounds__(256)
k_apply3d(const int32_t *__restrict__ map, const double *__restrict__ x,
          const double *__restrict__ qd, double *__restrict__ Ye, const Tab<D1, Q1> T,
          const int nblk, const KrylovState *__restrict__ st)
{
    if (st != nullptr && st->done) return;
    constexpr int ND = D1 * D1 * D1;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= nblk) return;

    // L->E gather (fused): 64 lanes read 256 contiguous bytes of map per local dof
    const int32_t *mp = map + (size_t)b * ND * kLanes + lane;
    double X[D1][D1][D1];
#pragma unroll
    for (int dz = 0; dz < D1; ++dz)
#pragma unroll
        for (int dy = 0; dy < D1; ++dy)
#pragma unroll
            for (int dx = 0; dx < D1; ++dx) {
                const int g = mp[(dx + D1 * (dy + D1 * dz)) * kLanes];
                if constexpr (CON) {
                    const double v = x[g < 0 ? 0 : g];
                    X[dz][dy][dx] = g < 0 ? 0.0 : v;
                } else {
                    X[dz][dy][dx] = x[g < 0 ? -g - 1 : g];
                }
            }

    double Y[D1][D1][D1];
    // AF: qd holds the block's affine factors [NC][kLanes] (pa_affine) or, AF 3, the geometry array
    // (pa_geom: header + [GeomLayout::kNC][kLanes] per block), else the per-point stream
    const double *q0 = qd_block<Q1, K, AF>(qd, b);
    auto xl = [&](int dz, int dy, int dx) { return X[dz][dy][dx]; };
    elem_apply3d_af<D1, Q1, K, AF>(xl, q0, lane, T, Y, qd);

    double *yp = Ye + (size_t)b * ND * kLanes + lane;
#pragma unroll
    for (int dz = 0; dz < D1; ++dz)
#pragma unroll
        for (int dy = 0; dy < D1; ++dy)
#pragma unroll
            for (int dx = 0; dx < D1; ++dx) yp[(dx + D1 * (dy + D1 * dz)) * kLanes] = Y[dz][dy][dx];
}

// ------------------------------------------------------------------------------------------------
// 2D apply (quads), same mapping
// ------------------------------------------------------------------------------------------------
template <int D1, int Q1, unsigned K, bool CON>
__global__ void __launch_bounds__(256)
k_apply2d(const int32_t *__restrict__ map, const double *__restrict__ x,
          const double *__restrict__ qd, double *__restrict__ Ye, const Tab<D1, Q1> T,
          const int nblk, const KrylovState *__restrict__ st)
{
    if (st != nullptr && st->done) return;
    using L = QLayout<K, 2>;
    constexpr int ND = D1 * D1;
    constexpr int NQ = Q1 * Q1;
    constexpr int NC = L::nc;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= nblk) return;

    const int32_t *mp = map + (size_t)b * ND * kLanes + lane;
    double X[D1][D1];
#pragma unroll
    for (int dy = 0; dy < D1; ++dy)
#pragma unroll
        for (int dx = 0; dx < D1; ++dx) {
            const int g = mp[(dx + D1 * dy) * kLanes];
            if constexpr (CON) {
                const double v = x[g < 0 ? 0 : g];
                X[dy][dx] = g < 0 ? 0.0 : v;
            } else {
                X[dy][dx] = x[g < 0 ? -g - 1 : g];
            }
        }
    double Y[D1][D1];
#pragma unroll
    for (int dy = 0; dy < D1; ++dy)
#pragma unroll
        for (int dx = 0; dx < D1; ++dx) Y[dy][dx] = 0.0;

    const double *q0 = qd + (size_t)b * NQ * NC * kLanes;
#pragma unroll
    for (int qy = 0; qy < Q1; ++qy) {
        double a[D1], ay[D1];
#pragma unroll
        for (int dx = 0; dx < D1; ++dx) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int dy = 0; dy < D1; ++dy) {
                s0 += T.B[qy][dy] * X[dy][dx];
                s1 += T.G[qy][dy] * X[dy][dx];
            }
            a[dx] = s0; ay[dx] = s1;
        }
        double Rv[D1], Ry[D1];
#pragma unroll
        for (int dx = 0; dx < D1; ++dx) { Rv[dx] = 0.0; Ry[dx] = 0.0; }
#pragma unroll
        for (int qx = 0; qx < Q1; ++qx) {
            double u = 0.0, ux = 0.0, uy = 0.0;
#pragma unroll
            for (int dx = 0; dx < D1; ++dx) {
                u += T.B[qx][dx] * a[dx];
                ux += T.G[qx][dx] * a[dx];
                uy += T.B[qx][dx] * ay[dx];
            }
            const int q = qx + Q1 * qy;
            double qv[NC];
            load_qp<NC, true>(q0 + (size_t)q * NC * kLanes, lane, qv);
            double vv = 0.0, gx = 0.0, gy = 0.0;
            if constexpr (L::kD) {
                gx = qv[0] * ux + qv[1] * uy;
                gy = qv[1] * ux + qv[2] * uy;
            }
            if constexpr (L::kC) vv = qv[L::oC] * ux + qv[L::oC + 1] * uy;
            if constexpr (L::kM) vv += qv[L::oM] * u;
#pragma unroll
            for (int dx = 0; dx < D1; ++dx) {
                if constexpr (L::kD) {
                    Rv[dx] += T.B[qx][dx] * vv + T.G[qx][dx] * gx;
                    Ry[dx] += T.B[qx][dx] * gy;
                } else {
                    Rv[dx] += T.B[qx][dx] * vv;
                }
            }
        }
#pragma unroll
        for (int dy = 0; dy < D1; ++dy)
#pragma unroll
            for (int dx = 0; dx < D1; ++dx) {
                if constexpr (L::kD)
                    Y[dy][dx] += T.B[qy][dy] * Rv[dx] + T.G[qy][dy] * Ry[dx];
                else
                    Y[dy][dx] += T.B[qy][dy] * Rv[dx];
            }
    }
    double *yp = Ye + (size_t)b * ND * kLanes + lane;
#pragma unroll
    for (int dy = 0; dy < D1; ++dy)
#pragma unroll
        for (int dx = 0; dx < D1; ++dx) yp[(dx + D1 * dy) * kLanes] = Y[dy][dx];
}

// ------------------------------------------------------------------------------------------------
// setup kernels (the multilinear map, its adjugate and the rule's points: point_geom.hpp)
// ------------------------------------------------------------------------------------------------
// qdata setup: thread per (element-block, q, lane); coalesced writes of the [b][q][c][lane] layout
template <int DIM>
__global__ void __launch_bounds__(256)
k_setup_qdata(const double *__restrict__ verts, const int32_t *__restrict__ perm, int ne, int nblk, int qlay,
              const Rule1D r, unsigned kinds,
              int nc, double kappa, const double *__restrict__ kappa_q, const double *__restrict__ kmat_q,
              double alpha, double c0, double c1, double c2, const double *__restrict__ conv_q, double mass,
              const double *__restrict__ mass_q, double *__restrict__ qd, double *__restrict__ gaff)
{
    const int q1 = r.q1;
    const int nq = DIM == 3 ? q1 * q1 * q1 : q1 * q1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)nblk * nq * kLanes) return;
    const int lane = (int)(t % kLanes);
    const int q = (int)((t / kLanes) % nq);
    const int b = (int)(t / ((int64_t)kLanes * nq));
    const int e = perm[(size_t)b * kLanes + lane];
    double *out = qd + ((size_t)b * nq + q) * nc * kLanes;
    // component k of this point: block layout (qd_offset) or element-major [e][k][q]
    auto put = [&](int k, double v) {
        if (qlay == 1) qd[qd_ho_index(e, k, q, nc, q1)] = v;
        else out[qd_offset(k, lane, nc)] = v;
    };
    // affine elements (gaff != nullptr, constant coefficients, block layout): J from the edge vectors
    // (the multilinear map's Jacobian, constant on a parallelepiped) and every stored point value
    // is W_q * g_k, with the per-element factor g_k also kept in gaff ([b][k][lane] on the block
    // layout, [e][k] on the high-order layout) for the kernels that form the point data themselves
    // (elem_apply3d<..., AFF>, k_apply3d_tile<..., MF & 16>)
    auto put_g = [&](int k, double W, double gk) {
        put(k, W * gk);
        if (q == 0) gaff[qlay == 1 ? (size_t)e * nc + k : ((size_t)b * nc + k) * kLanes + lane] = gk;
    };
    if (e < 0 || e >= ne) {
        if (qlay == 0)
            for (int k = 0; k < nc; ++k) out[qd_offset(k, lane, nc)] = 0.0;
        if (gaff && q == 0 && qlay == 0)
            for (int k = 0; k < nc; ++k) gaff[((size_t)b * nc + k) * kLanes + lane] = 0.0;
        return;
    }
    int qi[3];
    double xi[DIM], W;
    tensor_point<DIM>(q, q1, r, qi, xi, W);
    double J[DIM][DIM], A[DIM][DIM];
    const double *V = verts + (size_t)e * (1 << DIM) * DIM;
    if (gaff) {
        for (int i = 0; i < DIM; ++i)
            for (int k = 0; k < DIM; ++k) J[i][k] = V[(1 << k) * DIM + i] - V[i];
        const double det = adjugate<DIM>(J, A);
        int o = 0;
        if (kinds & CDFEM_DIFFUSION) {
            const double s = kappa / det;
            for (int i = 0; i < DIM; ++i)
                for (int j = i; j < DIM; ++j) {
                    double acc = 0.0;
                    for (int k = 0; k < DIM; ++k) acc += A[i][k] * A[j][k];
                    put_g(o++, W, s * acc);
                }
        }
        if (kinds & CDFEM_CONVECTION) {
            const double cv[3] = {c0, c1, c2};
            for (int i = 0; i < DIM; ++i) {
                double acc = 0.0;
                for (int k = 0; k < DIM; ++k) acc += A[i][k] * cv[k];
                put_g(o++, W, alpha * acc);
            }
        }
        if (kinds & CDFEM_MASS) put_g(o++, W, mass * det);
        return;
    }
    multilinear_map<DIM>(V, xi, J);
    const double det = adjugate<DIM>(J, A);
    const size_t eq = (size_t)e * nq + q;
    int o = 0;
    if (kinds & CDFEM_DIFFUSION) {
        const double kap = kappa_q ? kappa_q[eq] : kappa;
        if (kmat_q) {  // MatrixCoefficient: D = W adj(J) K adj(J)^T / det J, K = kap I + K_q (symmetric)
            constexpr int NS = DIM * (DIM + 1) / 2;
            double K[3][3];
            for (int k = 0, m = 0; k < DIM; ++k)
                for (int l = k; l < DIM; ++l, ++m) K[k][l] = K[l][k] = kmat_q[eq * NS + m] + (k == l ? kap : 0.0);
            const double s = W / det;
            for (int i = 0; i < DIM; ++i)
                for (int j = i; j < DIM; ++j) {
                    double acc = 0.0;
                    for (int k = 0; k < DIM; ++k) {
                        double t = 0.0;
                        for (int l = 0; l < DIM; ++l) t += K[k][l] * A[j][l];
                        acc += A[i][k] * t;
                    }
                    put(o++, s * acc);
                }
        } else {
            const double s = W * kap / det;
            for (int i = 0; i < DIM; ++i)
                for (int j = i; j < DIM; ++j) {
                    double acc = 0.0;
                    for (int k = 0; k < DIM; ++k) acc += A[i][k] * A[j][k];
                    put(o++, s * acc);
                }
        }
    }
    if (kinds & CDFEM_CONVECTION) {
        double cv[3] = {c0, c1, c2};
        if (conv_q)
            for (int k = 0; k < DIM; ++k) cv[k] = conv_q[eq * DIM + k];
        for (int i = 0; i < DIM; ++i) {
            double acc = 0.0;
            for (int k = 0; k < DIM; ++k) acc += A[i][k] * cv[k];
            put(o++, W * alpha * acc);
        }
    }
    if (kinds & CDFEM_MASS) {
        const double s = mass_q ? mass_q[eq] : mass;
        put(o++, W * s * det);
    }
}

// pa_geom: the per-element geometry of the AF 3 element core (pa_core.hpp GeomLayout), thread per
// (block, lane): the mask and the coefficients a1..a7 of the hex's trilinear map (lexicographic
// vertices: bit k of the vertex number = its position along axis k).  Padding lanes: the unit cube, mask 0.
__global__ void __launch_bounds__(256)
k_setup_geom(const double *__restrict__ verts, const int32_t *__restrict__ perm, int ne, int nblk,
             double *__restrict__ geom)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)nblk * kLanes) return;
    const int lane = (int)(t % kLanes), b = (int)(t / kLanes);
    const int e = perm[t];
    double *out = geom + GeomLayout::kHdr + (size_t)b * GeomLayout::kNC * kLanes + lane;
    const bool live = e >= 0 && e < ne;
    out[GeomLayout::oLive * kLanes] = live ? 1.0 : 0.0;
    const double *V = verts + (size_t)(live ? e : 0) * 24;
    for (int i = 0; i < 3; ++i) {
        const double v0 = V[i], v1 = V[3 + i], v2 = V[6 + i], v3 = V[9 + i];
        const double v4 = V[12 + i], v5 = V[15 + i], v6 = V[18 + i], v7 = V[21 + i];
        double a[7];
        a[0] = v1 - v0;
        a[1] = v2 - v0;
        a[2] = v4 - v0;
        a[3] = (v3 - v2) - (v1 - v0);
        a[4] = (v5 - v4) - (v1 - v0);
        a[5] = (v6 - v4) - (v2 - v0);
        a[6] = ((v7 - v6) - (v5 - v4)) - ((v3 - v2) - (v1 - v0));
        for (int m = 0; m < 7; ++m)
            out[(GeomLayout::oA + 3 * m + i) * kLanes] = live ? a[m] : (m == i ? 1.0 : 0.0);
    }
}

// ho_geom: the same coefficients (the same differences in the same order, so the two layouts hold the
// same values for the same element) element-major for the high-order tile apply (pa_core.hpp
// HoGeomLayout), thread per element
__global__ void __launch_bounds__(256)
k_setup_hgeom(const double *__restrict__ verts, int ne, double *__restrict__ geom)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    double *out = geom + GeomLayout::kHdr + (size_t)e * HoGeomLayout::kNC;
    const double *V = verts + (size_t)e * 24;
    for (int i = 0; i < 3; ++i) {
        const double v0 = V[i], v1 = V[3 + i], v2 = V[6 + i], v3 = V[9 + i];
        const double v4 = V[12 + i], v5 = V[15 + i], v6 = V[18 + i], v7 = V[21 + i];
        double a[7];
        a[0] = v1 - v0;
        a[1] = v2 - v0;
        a[2] = v4 - v0;
        a[3] = (v3 - v2) - (v1 - v0);
        a[4] = (v5 - v4) - (v1 - v0);
        a[5] = (v6 - v4) - (v2 - v0);
        a[6] = ((v7 - v6) - (v5 - v4)) - ((v3 - v2) - (v1 - v0));
        for (int m = 0; m < 7; ++m) out[3 * m + i] = a[m];
        out[21 + i] = 0.0;
    }
}

// physical coordinates of rule points: xyz[(e*nq + q)*dim + k]
template <int DIM>
__global__ void k_quad_points(const double *__restrict__ verts, int ne, const Rule1D r,
                              double *__restrict__ xyz)
{
    const int q1 = r.q1;
    const int nq = DIM == 3 ? q1 * q1 * q1 : q1 * q1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)ne * nq) return;
    const int e = (int)(t / nq), q = (int)(t % nq);
    int qi[3];
    double xi[DIM], W, x[DIM], J[DIM][DIM];
    tensor_point<DIM>(q, q1, r, qi, xi, W);
    multilinear_map<DIM>(verts + (size_t)e * (1 << DIM) * DIM, xi, J, x);
    for (int k = 0; k < DIM; ++k) xyz[t * DIM + k] = x[k];
}

// phi_l and reference gradient of local dof l at point q
__device__ inline void basis_at(int l, int q, int dim, const Rule1D &r, double &phi, double g[3])
{
    const int d1 = r.d1, q1 = r.q1;
    const int lx = l % d1, ly = (l / d1) % d1, lz = l / (d1 * d1);
    const int qx = q % q1, qy = (q / q1) % q1, qz = q / (q1 * q1);
    const double bx = r.B[qx][lx], gx = r.G[qx][lx], by = r.B[qy][ly], gy = r.G[qy][ly];
    if (dim == 2) {
        phi = bx * by; g[0] = gx * by; g[1] = bx * gy; g[2] = 0.0;
    } else {
        const double bz = r.B[qz][lz], gz = r.G[qz][lz];
        phi = bx * by * bz; g[0] = gx * by * bz; g[1] = bx * gy * bz; g[2] = bx * by * gz;
    }
}

// PA diagonal, element part: thread per (block, l, lane), Ye layout [b][l][lane]; element-major
// (qlay 1): thread per (e, l), Ye at ho_eidx(e, l)
template <int DIM>
__global__ void __launch_bounds__(256)
k_diag_elem(const double *__restrict__ qd, const int32_t *__restrict__ perm, int ne, int nblk, int nd, int qlay,
            const HoLayout ho, const Rule1D r, unsigned kinds, int nc, double *__restrict__ Ye)
{
    const int q1 = r.q1;
    const int nq = DIM == 3 ? q1 * q1 * q1 : q1 * q1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)nblk * nd * kLanes) return;
    // element blocks: lane = element; element-major (qlay 1): consecutive threads share an
    // element (l fastest), so every qdata read of a wave is one broadcast address
    const int lane = qlay == 1 ? 0 : (int)(t % kLanes);
    const int l = qlay == 1 ? (int)(t % nd) : (int)((t / kLanes) % nd);
    const int b = qlay == 1 ? 0 : (int)(t / ((int64_t)kLanes * nd));
    const int oC = (kinds & CDFEM_DIFFUSION) ? DIM * (DIM + 1) / 2 : 0;
    const int oM = oC + ((kinds & CDFEM_CONVECTION) ? DIM : 0);
    const int e = qlay == 1 ? (int)(t / nd) : perm[(size_t)b * kLanes + lane];
    if (qlay == 1 && e >= ne) return;
    double acc = 0.0;
    for (int q = 0; q < nq; ++q) {
        const double *qb = qd + ((size_t)b * nq + q) * nc * kLanes;
        auto qq = [&](int k) {
            return qlay == 1 ? qd[qd_ho_index(e, k, q, nc, q1)] : qb[qd_offset(k, lane, nc)];
        };
        double phi, g[3];
        basis_at(l, q, DIM, r, phi, g);
        if (kinds & CDFEM_DIFFUSION) {
            if (DIM == 3) {
                const double d00 = qq(0), d01 = qq(1), d02 = qq(2);
                const double d11 = qq(3), d12 = qq(4), d22 = qq(5);
                acc += g[0] * (d00 * g[0] + d01 * g[1] + d02 * g[2]) +
                       g[1] * (d01 * g[0] + d11 * g[1] + d12 * g[2]) +
                       g[2] * (d02 * g[0] + d12 * g[1] + d22 * g[2]);
            } else {
                const double d00 = qq(0), d01 = qq(1), d11 = qq(2);
                acc += g[0] * (d00 * g[0] + d01 * g[1]) + g[1] * (d01 * g[0] + d11 * g[1]);
            }
        }
        if (kinds & CDFEM_CONVECTION) {
            double cg = 0.0;
            for (int k = 0; k < DIM; ++k) cg += qq(oC + k) * g[k];
            acc += phi * cg;
        }
        if (kinds & CDFEM_MASS) acc += qq(oM) * phi * phi;
    }
    if (qlay == 1) Ye[ho_eidx(ho, (uint32_t)e, l)] = acc;
    else Ye[t] = acc;  // t == (b*nd + l)*64 + lane
}

// PA diagonal, sum-factorised (MFEM's PA AssembleDiagonal): thread per (element, i1[, i2]) computing
// the D1 entries along the last axis.  Every term of the operator is a qdata component c times a
// product of 1D factors, one per axis: F_d(q, i) = u_d(q, i) v_d(q, i) with u, v = G when the term
// differentiates along d, else B, so
//   diag(i) = sum_terms mult * sum_{q_last} F_last * (... sum_{q1} F_1 * qd_c(q)).
// Terms (DiagTerms): diffusion c = (a, b) with a <= b (off-diagonal twice), convection c = oC + k
// with (k, none), mass (none, none).  Everything (term list, sizes, factor types) is compile-time:
// the loops unroll and no array is indexed at run time (no scratch).  The D1^(dim-1) threads of an
// element are consecutive, so each qdata load of a wave is a broadcast of at most a few addresses
// and an element's qdata is fetched from HBM once.  10 Q1^dim FMAs per thread and term class
// against D1^dim Q1^dim for the per-entry form (k_diag_elem, kept for rules other than the
// operators' n = p + 2).
template <int DIM, unsigned K>
struct DiagTerms {
    static constexpr int nD = (K & CDFEM_DIFFUSION) ? DIM * (DIM + 1) / 2 : 0;
    static constexpr int nC = (K & CDFEM_CONVECTION) ? DIM : 0;
    static constexpr int n = nD + nC + ((K & CDFEM_MASS) ? 1 : 0);
    // derivative axes a <= b of diffusion term t (components D00, D01, D02, D11, D12, D22 / D00, D01, D11)
    static constexpr int da(int t) { return DIM == 3 ? (t < 3 ? 0 : t < 5 ? 1 : 2) : (t < 2 ? 0 : 1); }
    static constexpr int db(int t) { return DIM == 3 ? (t < 3 ? t : t < 5 ? t - 2 : 2) : (t < 2 ? t : 1); }
    static constexpr int a(int t) { return t < nD ? da(t) : t < nD + nC ? t - nD : -1; }
    static constexpr int b(int t) { return t < nD ? db(t) : -1; }
    static constexpr double mult(int t) { return t < nD && da(t) != db(t) ? 2.0 : 1.0; }
    // qdata component of term t (its index in QLayout order: D, then C, then M)
    static constexpr int comp(int t) { return t; }
    // 1D factor along axis d: 0 = B B, 1 = G B, 2 = G G
    static constexpr int type(int t, int d) { return (a(t) == d ? 1 : 0) + (b(t) == d ? 1 : 0); }
};

template <int D1, int Q1>
__device__ __forceinline__ double diag_factor(const Tab<D1, Q1> &T, int type, int q, int i)
{
    const double bq = T.B[q][i], gq = T.G[q][i];
    return type == 0 ? bq * bq : type == 1 ? gq * bq : gq * gq;
}

template <int DIM, int D1, int Q1, unsigned K>
__global__ void __launch_bounds__(256)
k_diag_sf(const double *__restrict__ qd, const int32_t *__restrict__ perm, int ne, int nblk, int qlay,
          const HoLayout ho, const Tab<D1, Q1> T, double *__restrict__ Ye)
{
    using TT = DiagTerms<DIM, K>;
    constexpr int NC = QLayout<K, DIM>::nc;
    constexpr int ND = DIM == 3 ? D1 * D1 * D1 : D1 * D1;
    constexpr int NQ = DIM == 3 ? Q1 * Q1 * Q1 : Q1 * Q1;
    constexpr int NT = DIM == 3 ? D1 * D1 : D1;  // threads per element
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t npos = qlay == 1 ? (int64_t)ne : (int64_t)nblk * kLanes;
    if (t >= npos * NT) return;
    const int64_t pos = t / NT;
    const int it = (int)(t - pos * NT);
    const int i1 = it % D1, i2 = DIM == 3 ? it / D1 : 0;
    const int b = qlay == 1 ? 0 : (int)(pos / kLanes), lane = qlay == 1 ? 0 : (int)(pos % kLanes);
    const int e = qlay == 1 ? (int)pos : perm[pos];
    auto out = [&](int i3, double v) {
        const int l = DIM == 3 ? i1 + D1 * (i2 + D1 * i3) : i1 + D1 * i3;
        if (qlay == 1) Ye[ho_eidx(ho, (uint32_t)e, l)] = v;
        else Ye[((size_t)b * ND + l) * kLanes + lane] = v;
    };
    if (e < 0 || e >= ne) {
#pragma unroll
        for (int i3 = 0; i3 < D1; ++i3) out(i3, 0.0);
        return;
    }
    // qdata of component c at (qx, qy[, qz]): base_c + qz * sz + (qx + Q1 qy) * sxy
    const size_t plane = qd_ho_plane(NC, Q1);
    auto cbase = [&](int c, size_t &sxy, size_t &sz) -> const double * {
        if (qlay == 1) {
            constexpr int QQ = Q1 * Q1;
            const bool pair = c < (NC & ~1);
            sxy = pair ? 2 : 1;
            sz = DIM == 3 ? plane : 0;
            return qd + (size_t)e * Q1 * plane + (pair ? (size_t)(c >> 1) * QQ * 2 + (c & 1) : (size_t)(NC & ~1) * QQ);
        }
        sxy = (size_t)NC * kLanes;
        sz = (size_t)Q1 * Q1 * NC * kLanes;
        return qd + (size_t)b * NQ * NC * kLanes + qd_offset(c, lane, NC);
    };
    constexpr int last = DIM - 1;
    double acc[D1];
#pragma unroll
    for (int i3 = 0; i3 < D1; ++i3) acc[i3] = 0.0;
#pragma unroll
    for (int s = 0; s < TT::n; ++s) {
        size_t sxy = 0, sz = 0;
        const double *qc = cbase(TT::comp(s), sxy, sz);
        double f1[Q1], f2[Q1];
#pragma unroll
        for (int q = 0; q < Q1; ++q) {
            f1[q] = diag_factor(T, TT::type(s, 0), q, i1);
            f2[q] = DIM == 3 ? diag_factor(T, TT::type(s, 1), q, i2) : 0.0;
        }
        // the last axis' quadrature index: not unrolled in 3D, so one plane's Q1^2 loads are in
        // flight per step (fully unrolled, the compiler hoists all Q1^3 loads: up to 256 VGPRs + spills)
        constexpr int kUz = DIM == 3 ? 1 : Q1;
#pragma unroll kUz
        for (int qz = 0; qz < Q1; ++qz) {
            double szs = 0.0;
            if constexpr (DIM == 3) {
                const double *qp = qc + qz * sz;
#pragma unroll
                for (int qy = 0; qy < Q1; ++qy) {
                    double sx = 0.0;
#pragma unroll
                    for (int qx = 0; qx < Q1; ++qx) sx += f1[qx] * qp[(size_t)(qx + Q1 * qy) * sxy];
                    szs += f2[qy] * sx;
                }
            } else {
#pragma unroll
                for (int qx = 0; qx < Q1; ++qx) szs += f1[qx] * qc[(size_t)(qx + Q1 * qz) * sxy];
            }
            szs *= TT::mult(s);
#pragma unroll
            for (int i3 = 0; i3 < D1; ++i3) acc[i3] += diag_factor(T, TT::type(s, last), qz, i3) * szs;
        }
    }
#pragma unroll
    for (int i3 = 0; i3 < D1; ++i3) out(i3, acc[i3]);
}

// PA diagonal on the element-major high-order layout (3D, qlay 1: p = 3, 4), sum-factorised in three
// stages with LDS between them, so every qdata value is read from HBM exactly once, by one thread:
//   1. thread (e, qx, qy) loads its point column (all qz, all components: the tile apply's 16-byte
//      loads) and contracts z: A_g(qx, qy, dz) = sum_{t in g} mult_t sum_qz F_z^t(qz, dz) qd_t(q);
//      terms are grouped by their (x, y) factor types g = (tx, ty) (at most 6 groups for D+C+M)
//   2. per group, through LDS, thread (e, qx, dz) contracts y into S_tx(qx, dy, dz)
//   3. thread (e, dy, dz) contracts x: diag(dx, dy, dz) = sum_tx sum_qx F_x^tx(qx, dx) S_tx.
// Term list, sizes and factor types are compile-time (DiagTerms); ~4 KB of LDS per element.
template <unsigned K>
__host__ __device__ constexpr bool diag_slot_used(int slot)
{
    for (int t = 0; t < DiagTerms<3, K>::n; ++t)
        if (3 * DiagTerms<3, K>::type(t, 0) + DiagTerms<3, K>::type(t, 1) == slot) return true;
    return false;
}

template <int D1, int Q1, unsigned K>
__global__ void __launch_bounds__(256)
k_diag_ho(const double *__restrict__ qd, int ne, const HoLayout ho, const Tab<D1, Q1> T, double *__restrict__ Ye)
{
    using TT = DiagTerms<3, K>;
    constexpr int NC = QLayout<K, 3>::nc, NP = NC / 2, QQ = Q1 * Q1;
    constexpr int PS = qd_ho_plane(NC, Q1);
    constexpr int EPB = 256 / QQ;
    __shared__ double sA[EPB][D1][QQ];            // one group's z-contracted column sums
    __shared__ double sS[3][EPB][D1][D1][Q1];     // y-contracted sums per x factor type
    const int tid = threadIdx.x;
    // ---- stage 1: thread (le, qx + Q1 qy)
    const int le1 = tid / QQ, t1 = tid - le1 * QQ;
    const int e1 = blockIdx.x * EPB + le1;
    const bool v1 = le1 < EPB && e1 < ne;
    double qv[Q1][NC];
    {
        const double *qe = qd + (size_t)(v1 ? e1 : ne - 1) * Q1 * PS;
        const int tc = v1 ? t1 : 0;
#pragma unroll
        for (int qz = 0; qz < Q1; ++qz) {
            const double *qp = qe + qz * PS;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const v2d_t w = __builtin_nontemporal_load(reinterpret_cast<const v2d_t *>(qp + p * 2 * QQ) + tc);
                qv[qz][2 * p] = w.x;
                qv[qz][2 * p + 1] = w.y;
            }
            if constexpr (NC & 1) qv[qz][NC - 1] = __builtin_nontemporal_load(qp + 2 * NP * QQ + tc);
        }
    }
    double A[9][D1];
#pragma unroll
    for (int g = 0; g < 9; ++g)
#pragma unroll
        for (int dz = 0; dz < D1; ++dz) A[g][dz] = 0.0;
#pragma unroll
    for (int t = 0; t < TT::n; ++t) {
        const int g = 3 * TT::type(t, 0) + TT::type(t, 1), tz = TT::type(t, 2);
#pragma unroll
        for (int qz = 0; qz < Q1; ++qz) {
            const double v = TT::mult(t) * qv[qz][TT::comp(t)];
#pragma unroll
            for (int dz = 0; dz < D1; ++dz) A[g][dz] += diag_factor(T, tz, qz, dz) * v;
        }
    }
    // ---- stage 2, group by group: thread (le, qx, dz)
    const int le2 = tid / (Q1 * D1), r2 = tid - le2 * (Q1 * D1);
    const int qx2 = r2 % Q1, dz2 = r2 / Q1;
    const bool v2 = le2 < EPB;
    double S[3][D1];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int dy = 0; dy < D1; ++dy) S[x][dy] = 0.0;
#pragma unroll
    for (int g = 0; g < 9; ++g) {
        if (!diag_slot_used<K>(g)) continue;  // compile-time after unrolling
        if (le1 < EPB)
#pragma unroll
            for (int dz = 0; dz < D1; ++dz) sA[le1][dz][t1] = A[g][dz];
        __syncthreads();
        if (v2) {
            const int tx = g / 3, ty = g % 3;
#pragma unroll
            for (int qy = 0; qy < Q1; ++qy) {
                const double a = sA[le2][dz2][qx2 + Q1 * qy];
#pragma unroll
                for (int dy = 0; dy < D1; ++dy) S[tx][dy] += diag_factor(T, ty, qy, dy) * a;
            }
        }
        __syncthreads();
    }
    if (v2)
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int dy = 0; dy < D1; ++dy) sS[x][le2][dz2][dy][qx2] = S[x][dy];
    __syncthreads();
    // ---- stage 3: thread (le, dy, dz)
    const int le3 = tid / (D1 * D1), r3 = tid - le3 * (D1 * D1);
    const int dy3 = r3 % D1, dz3 = r3 / D1;
    const int e3 = blockIdx.x * EPB + le3;
    if (le3 >= EPB || e3 >= ne) return;
    double out[D1];
#pragma unroll
    for (int dx = 0; dx < D1; ++dx) out[dx] = 0.0;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        bool used = false;
#pragma unroll
        for (int y = 0; y < 3; ++y) used = used || diag_slot_used<K>(3 * x + y);
        if (!used) continue;
#pragma unroll
        for (int qx = 0; qx < Q1; ++qx) {
            const double sv = sS[x][le3][dz3][dy3][qx];
#pragma unroll
            for (int dx = 0; dx < D1; ++dx) out[dx] += diag_factor(T, x, qx, dx) * sv;
        }
    }
#pragma unroll
    for (int dx = 0; dx < D1; ++dx) Ye[ho_eidx(ho, (uint32_t)e3, dx + D1 * (dy3 + D1 * dz3))] = out[dx];
}

// linear form, element part: be_l = sum_q W detJ f_q phi_l; thread per (block, l, lane)
template <int DIM>
__global__ void __launch_bounds__(256)
k_lf_elem(const double *__restrict__ verts, const int32_t *__restrict__ perm, int ne, int nblk, int nd, int qlay,
          const HoLayout ho, const Rule1D r,
          const double *__restrict__ fq, double *__restrict__ Ye)
{
    const int q1 = r.q1;
    const int nq = DIM == 3 ? q1 * q1 * q1 : q1 * q1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)nblk * nd * kLanes) return;
    // element-major (qlay 1): thread per (e, l), l fastest (as k_diag_elem)
    const int lane = qlay == 1 ? 0 : (int)(t % kLanes);
    const int l = qlay == 1 ? (int)(t % nd) : (int)((t / kLanes) % nd);
    const int b = qlay == 1 ? 0 : (int)(t / ((int64_t)kLanes * nd));
    const int e = qlay == 1 ? (int)(t / nd) : perm[(size_t)b * kLanes + lane];
    double acc = 0.0;
    if (e >= 0 && e < ne) {
        for (int q = 0; q < nq; ++q) {
            int qi[3];
            double xi[DIM], W, J[DIM][DIM], A[DIM][DIM], phi, g[3];
            tensor_point<DIM>(q, q1, r, qi, xi, W);
            multilinear_map<DIM>(verts + (size_t)e * (1 << DIM) * DIM, xi, J);
            const double det = adjugate<DIM>(J, A);
            basis_at(l, q, DIM, r, phi, g);
            acc += W * det * fq[(size_t)e * nq + q] * phi;
        }
    }
    if (qlay == 1) {
        if (e >= 0 && e < ne) Ye[ho_eidx(ho, (uint32_t)e, l)] = acc;
    } else {
        Ye[t] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline unsigned grid_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

hipError_t launch_setup_qdata(cdfem_ctx *c, const double *d_kappa_q, const double *d_kmat_q, double kappa, double alpha,
                              const double *conv, const double *d_conv_q, const double *d_mass_q,
                              double mass)
{
    const int q1 = c->rule_op.q1;
    const int nq = c->dim == 3 ? q1 * q1 * q1 : q1 * q1;
    const int64_t n = (int64_t)c->nblk * nq * kLanes;
    const double c0 = conv ? conv[0] : 0.0, c1 = conv ? conv[1] : 0.0;
    const double c2 = (conv && c->dim == 3) ? conv[2] : 0.0;
    if (c->dim == 3)
        hipLaunchKernelGGL(k_setup_qdata<3>, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           c->d_verts, c->d_perm, c->ne, c->nblk, c->qlay, c->rule_op, c->kinds, c->ncomp, kappa,
                           d_kappa_q, d_kmat_q, alpha, c0, c1, c2, d_conv_q, mass, d_mass_q, c->d_qd, c->d_qaff);
    else
        hipLaunchKernelGGL(k_setup_qdata<2>, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           c->d_verts, c->d_perm, c->ne, c->nblk, c->qlay, c->rule_op, c->kinds, c->ncomp, kappa,
                           d_kappa_q, d_kmat_q, alpha, c0, c1, c2, d_conv_q, mass, d_mass_q, c->d_qd, c->d_qaff);
    return hipGetLastError();
}

hipError_t launch_setup_geom(cdfem_ctx *c)
{
    const int64_t n = (int64_t)c->nblk * kLanes;
    hipLaunchKernelGGL(k_setup_geom, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->d_verts, c->d_perm, c->ne,
                       c->nblk, c->d_geom);
    return hipGetLastError();
}

hipError_t launch_setup_hgeom(cdfem_ctx *c)
{
    hipLaunchKernelGGL(k_setup_hgeom, dim3(grid_for(c->ne, 256)), dim3(256), 0, c->stream, c->d_verts, (int)c->ne,
                       c->d_hgeom);
    return hipGetLastError();
}

hipError_t launch_quad_points(cdfem_ctx *c, const Rule1D &r, double *xyz)
{
    const int nq = c->dim == 3 ? r.q1 * r.q1 * r.q1 : r.q1 * r.q1;
    const int64_t n = (int64_t)c->ne * nq;
    if (c->dim == 3)
        hipLaunchKernelGGL(k_quad_points<3>, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           c->d_verts, c->ne, r, xyz);
    else
        hipLaunchKernelGGL(k_quad_points<2>, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           c->d_verts, c->ne, r, xyz);
    return hipGetLastError();
}

template <int D1, int Q1>
static bool diag_ho_kinds(cdfem_ctx *c, double *Ye)
{
    constexpr int EPB = 256 / (Q1 * Q1);
    const dim3 g((unsigned)((c->ne + EPB - 1) / EPB)), bs(256);
    const Tab<D1, Q1> T = make_tab<D1, Q1>(c->rule_op);
    return dispatch_kinds(c->kinds, false, [&](auto K) {
        hipLaunchKernelGGL((k_diag_ho<D1, Q1, K()>), g, bs, 0, c->stream, c->d_qd, c->ne, ho_layout(c), T, Ye);
        return true;
    });
}

template <int DIM, int D1, int Q1>
static bool diag_sf_kinds(cdfem_ctx *c, double *Ye)
{
    const int64_t npos = c->qlay == 1 ? (int64_t)c->ne : (int64_t)c->nblk * kLanes;
    const int64_t n = npos * (DIM == 3 ? D1 * D1 : D1);
    const dim3 g(grid_for(n, 256)), bs(256);
    const Tab<D1, Q1> T = make_tab<D1, Q1>(c->rule_op);
    return dispatch_kinds(c->kinds, false, [&](auto K) {
        hipLaunchKernelGGL((k_diag_sf<DIM, D1, Q1, K()>), g, bs, 0, c->stream, c->d_qd, c->d_perm, c->ne, c->nblk,
                           c->qlay, ho_layout(c), T, Ye);
        return true;
    });
}

hipError_t launch_diag_elem(cdfem_ctx *c, double *Ye)
{
    if (nl_jac_current(c)) return launch_nl_tensor(c, 2, c->heat.d_ulin, nullptr, false, Ye, nullptr);
    const int d1 = c->rule_op.d1, q1 = c->rule_op.q1;
    bool done = false;
    if (d1 == q1 - 1) {  // the operators' Gauss n = p + 2 rules: sum-factorised, compile-time sizes
        done = dispatch_value<2, 3, 4, 5>(d1, false, [&](auto D1) {
            if (c->dim != 3) return diag_sf_kinds<2, D1(), D1() + 1>(c, Ye);
            if constexpr (D1() >= 4) {  // p = 3, 4 in the element-major layout: the tile kernel
                if (c->qlay == 1) return diag_ho_kinds<D1(), D1() + 1>(c, Ye);
            }
            return diag_sf_kinds<3, D1(), D1() + 1>(c, Ye);
        });
    }
    if (done) return hipGetLastError();
    // any other rule: the per-entry quadrature loop
    const int64_t n = (int64_t)c->nblk * c->nd * kLanes;
    if (c->dim == 3)
        hipLaunchKernelGGL(k_diag_elem<3>, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           c->d_qd, c->d_perm, c->ne, c->nblk, c->nd, c->qlay, ho_layout(c), c->rule_op, c->kinds, c->ncomp, Ye);
    else
        hipLaunchKernelGGL(k_diag_elem<2>, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           c->d_qd, c->d_perm, c->ne, c->nblk, c->nd, c->qlay, ho_layout(c), c->rule_op, c->kinds, c->ncomp, Ye);
    return hipGetLastError();
}

hipError_t launch_lf_elem(cdfem_ctx *c, const double *d_fq, double *Ye)
{
    const int64_t n = (int64_t)c->nblk * c->nd * kLanes;
    if (c->dim == 3)
        hipLaunchKernelGGL(k_lf_elem<3>, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           c->d_verts, c->d_perm, c->ne, c->nblk, c->nd, c->qlay, ho_layout(c), c->rule_lf, d_fq, Ye);
    else
        hipLaunchKernelGGL(k_lf_elem<2>, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           c->d_verts, c->d_perm, c->ne, c->nblk, c->nd, c->qlay, ho_layout(c), c->rule_lf, d_fq, Ye);
    return hipGetLastError();
}

template <int DIM, int D1, int Q1>
static hipError_t apply_dq(cdfem_ctx *c, const double *x, double *Ye, bool con, const KrylovState *st)
{
    const Tab<D1, Q1> T = make_tab<D1, Q1>(c->rule_op);
    const dim3 grid(grid_for(c->nblk, 4)), block(256);
    const int af = DIM == 3 ? pa_form(c) : 0;
    const double *qd = af == 3 ? c->d_geom : af ? c->d_qaff : c->d_qd;
    return dispatch_kinds(c->kinds, hipErrorInvalidValue, [&](auto K) {
        return dispatch_bools(con, [&](auto CON) {
            if constexpr (DIM == 3) {
                return dispatch_value<0, 1, 2, 3>(af, hipErrorInvalidValue, [&](auto AF) {
                    hipLaunchKernelGGL((k_apply3d<D1, Q1, K(), CON(), AF()>), grid, block, 0, c->stream, c->d_map, x,
                                       qd, Ye, T, c->nblk, st);
                    return hipGetLastError();
                });
            } else {
                hipLaunchKernelGGL((k_apply2d<D1, Q1, K(), CON()>), grid, block, 0, c->stream, c->d_map, x, qd, Ye,
                                   T, c->nblk, st);
                return hipGetLastError();
            }
        });
    });
}

bool apply_supported(int dim, int p)
{
    if (dim == 3) return p >= 1 && p <= 4;  // p = 3, 4: wave per element (ho_kernels.hip)
    if (dim == 2) return p >= 1 && p <= 4;
    return false;
}

// the kernel-side CG loop passes its state so a finished solve turns queued launches into no-ops
hipError_t launch_apply_st(cdfem_ctx *c, const double *x, double *Ye, bool con, const KrylovState *st)
{
    if (nl_jac_current(c)) return launch_nl_tensor(c, 1, c->heat.d_ulin, x, con, Ye, st);  // J(u) x, matrix-free
    const int q1 = c->rule_op.q1;
    if (c->dim == 3) {  // the Gauss rule of p + 2 points; p = 3, 4: wave per element (ho_kernels.hip)
        if (c->p >= 3) return launch_apply_wpe(c, x, Ye, con, st);
        if (q1 != c->p + 2) return hipErrorInvalidValue;
        return dispatch_value<1, 2>(c->p, hipErrorInvalidValue,
                                    [&](auto P) { return apply_dq<3, P() + 1, P() + 2>(c, x, Ye, con, st); });
    }
    if (q1 != c->p + 1) return hipErrorInvalidValue;  // 2D: p + 1 points
    return dispatch_value<1, 2, 3, 4>(c->p, hipErrorInvalidValue,
                                      [&](auto P) { return apply_dq<2, P() + 1, P() + 1>(c, x, Ye, con, st); });
}

hipError_t launch_apply(cdfem_ctx *c, const double *x, double *Ye, bool constrained)
{
    return launch_apply_st(c, x, Ye, constrained, nullptr);
}

}  // namespace cdfem
