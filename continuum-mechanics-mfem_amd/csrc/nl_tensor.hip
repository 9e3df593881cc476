// nl_tensor.hip — the quasi-linear backward-Euler heat form of nl_kernels.hip on quads and hexes, matrix-free:
// the residual, the Jacobian action J(u) v and the Jacobian diagonal, with no stored quadrature data.
//
//   a(u) = a0 + a1 (u - u_ref),  m(u) = m0 + m1 (u - u_ref),  W = w_q det J_q,
//   R_i     = sum_q W [ m(u) (u - u_old) / dt phi_i + a(u) grad u . grad phi_i ]
//   (J v)_i = sum_q W [ (m(u) + m1 (u - u_old)) / dt v phi_i + (a(u) grad v + a1 v grad u) . grad phi_i ]
//   J_ii    = sum_q W [ (m(u) + m1 (u - u_old)) / dt phi_i^2 + a(u) |grad phi_i|^2 + a1 phi_i (grad phi_i . grad u) ]
//
// The rule is tensor Gauss-Legendre with Q1 = p + 2 (quads) / p + 3 (hexes) points per direction (MFEM's
// IntRules.Get(geom, 2p + OrderW + 2)); the geometry is the multilinear map of the element's 2^dim
// vertices, its adj(J) and det J formed at every point.
//
// k_nl_tensor<DIM, P, MODE>: a Q1 x Q1 thread tile per element, EPB = 256 / Q1^2 elements per workgroup.
//   1. the element's dofs of u, u - u_old (the difference per dof, before the interpolation) and v, and its
//      vertices, into LDS;
//   2. thread (qx, qy) contracts x and y for every dz into registers (a column of points along z), then walks
//      the z points: the fields and their reference gradients at the point, the point's geometry, the point
//      operator, and the transposed z contraction into per-dz accumulators.  grad u is taken of u - u(dof 0)
//      (nl_kernels.hip nl_point says why);
//   3. the accumulators pass through LDS, and the transposed x / y contraction gives every local dof's entry:
//      one fixed summation order, the E-vector written in the context's layout ([block][dof][64]) and summed
//      by k_e2l in ascending element order.  No atomics.
// 2D is the same kernel with one z plane.  The diagonal mode keeps six accumulators per dz, one for each
// pattern of B and G in x and y that a term of J_ii has.
#include <hip/hip_runtime.h>

#include "cdfem_internal.hpp"
#include "point_geom.hpp"

namespace cdfem {

enum : int { kNlResidual = 0, kNlJvp = 1, kNlDiag = 2 };

template <int D1, int Q1>
struct NlTab {
    double B[Q1][D1];
    double G[Q1][D1];
    double pts[Q1];
    double w[Q1];
};

template <int DIM, int P>
struct NlShape : TensorShape<DIM, P, nl_tensor_points_1d(DIM, P)> {
    using TensorShape<DIM, P, nl_tensor_points_1d(DIM, P)>::Q1;
    static constexpr int TPE = Q1 * Q1;     // threads per element
    static constexpr int EPB = 256 / TPE;   // elements per workgroup
    static constexpr int NT = EPB * TPE;    // live threads of the workgroup
};

// slots: the element slots of the context's layout (64 per block; perm[slot] = element, -1 = padding)
template <int DIM, int P, int MODE>
__global__ void __launch_bounds__(256)
k_nl_tensor(const int32_t *__restrict__ map, const int32_t *__restrict__ perm, const double *__restrict__ verts,
            int nslots, const NlTab<P + 1, nl_tensor_points_1d(DIM, P)> T, cdfem_nl_heat_coeffs k,
            const double *__restrict__ u, const double *__restrict__ uold, const double *__restrict__ v, int con,
            double *__restrict__ Ye, const KrylovState *__restrict__ st)
{
    if (st != nullptr && st->done) return;
    using S = NlShape<DIM, P>;
    constexpr int D1 = S::D1, Q1 = S::Q1, D1Z = S::DZ, Q1Z = S::QZ, ND = S::ND, NV = S::NV, TPE = S::TPE,
                  EPB = S::EPB, NT = S::NT;
    constexpr int NP = MODE == kNlDiag ? 6 : 3;   // accumulators per dz
    constexpr int NF = MODE == kNlJvp ? 3 : 2;    // fields in LDS: u, u - u_old, v
    __shared__ double sB[Q1][D1], sG[Q1][D1], sPts[Q1], sW[Q1];
    __shared__ double sF[NF][EPB][ND];
    __shared__ double sX[EPB][NV * DIM];
    __shared__ double sP[EPB][NP][D1Z][TPE];
    __shared__ int sE[EPB];

    const int t = threadIdx.x;
    const int slot0 = blockIdx.x * EPB;
    for (int i = t; i < Q1 * D1; i += 256) {
        sB[i / D1][i % D1] = T.B[i / D1][i % D1];
        sG[i / D1][i % D1] = T.G[i / D1][i % D1];
    }
    if (t < Q1) {
        sPts[t] = T.pts[t];
        sW[t] = T.w[t];
    }
    if (t < EPB) sE[t] = slot0 + t < nslots ? perm[slot0 + t] : -1;
    __syncthreads();
    // 1. the elements' dofs and vertices
    for (int i = t; i < EPB * ND; i += 256) {
        const int el = i / ND, l = i - el * ND;
        if (sE[el] < 0) continue;
        const int slot = slot0 + el;
        const int32_t m = map[((size_t)(slot >> 6) * ND + l) * kLanes + (slot & 63)];
        const int32_t g = m < 0 ? -m - 1 : m;
        const double uu = u[g];
        sF[0][el][l] = uu;
        sF[1][el][l] = uu - uold[g];
        if constexpr (MODE == kNlJvp) {
            const double vv = v[g];
            sF[2][el][l] = (con && m < 0) ? 0.0 : vv;
        }
    }
    for (int i = t; i < EPB * NV * DIM; i += 256) {
        const int el = i / (NV * DIM), j = i - el * (NV * DIM);
        if (sE[el] >= 0) sX[el][j] = verts[(size_t)sE[el] * NV * DIM + j];
    }
    __syncthreads();

    const int el = t / TPE, r = t - el * TPE;
    const bool live = t < NT && sE[el < EPB ? el : 0] >= 0;
    if (live) {
        const int qx = r % Q1, qy = r / Q1;
        // 2a. x and y contractions for every dz: value, the same of u - u(dof 0), d/dxi, d/deta
        double uv[D1Z], uw[D1Z], ugx[D1Z], ugy[D1Z], dv[D1Z];
        double vv[D1Z], vgx[D1Z], vgy[D1Z];
        {
            double bx[D1], gx[D1], by[D1], gy[D1];
#pragma unroll
            for (int d = 0; d < D1; ++d) {
                bx[d] = sB[qx][d];
                gx[d] = sG[qx][d];
                by[d] = sB[qy][d];
                gy[d] = sG[qy][d];
            }
            const double u0 = sF[0][el][0];
#pragma unroll
            for (int dz = 0; dz < D1Z; ++dz) {
                uv[dz] = uw[dz] = ugx[dz] = ugy[dz] = dv[dz] = 0.0;
                vv[dz] = vgx[dz] = vgy[dz] = 0.0;
#pragma unroll
                for (int dy = 0; dy < D1; ++dy) {
                    double s = 0.0, s0 = 0.0, s1 = 0.0, sd = 0.0, sv = 0.0, sv1 = 0.0;
#pragma unroll
                    for (int dx = 0; dx < D1; ++dx) {
                        const int l = dx + D1 * (dy + D1 * dz);
                        const double ul = sF[0][el][l], wl = ul - u0;
                        s += bx[dx] * ul;
                        s0 += bx[dx] * wl;
                        s1 += gx[dx] * wl;
                        sd += bx[dx] * sF[1][el][l];
                        if constexpr (MODE == kNlJvp) {
                            const double vl = sF[2][el][l];
                            sv += bx[dx] * vl;
                            sv1 += gx[dx] * vl;
                        }
                    }
                    uv[dz] += by[dy] * s;
                    uw[dz] += by[dy] * s0;
                    ugx[dz] += by[dy] * s1;
                    ugy[dz] += gy[dy] * s0;
                    dv[dz] += by[dy] * sd;
                    if constexpr (MODE == kNlJvp) {
                        vv[dz] += by[dy] * sv;
                        vgx[dz] += by[dy] * sv1;
                        vgy[dz] += gy[dy] * sv;
                    }
                }
            }
        }
        // 2b. the column's geometry: the map's xi and eta derivatives on the z = 0 and z = 1 faces, and its
        // zeta derivative (constant along the column)
        const double xi = sPts[qx], eta = sPts[qy];
        double Jx[2][DIM], Jy[2][DIM];
        [[maybe_unused]] double Jz[DIM];
        {
            const double *V = sX[el];
#pragma unroll
            for (int f = 0; f < (DIM == 3 ? 2 : 1); ++f)
#pragma unroll
                for (int i = 0; i < DIM; ++i) {
                    const double v00 = V[(4 * f + 0) * DIM + i], v10 = V[(4 * f + 1) * DIM + i],
                                 v01 = V[(4 * f + 2) * DIM + i], v11 = V[(4 * f + 3) * DIM + i];
                    Jx[f][i] = (1.0 - eta) * (v10 - v00) + eta * (v11 - v01);
                    Jy[f][i] = (1.0 - xi) * (v01 - v00) + xi * (v11 - v10);
                    if constexpr (DIM == 3) {
                        const double pf = (1.0 - eta) * ((1.0 - xi) * v00 + xi * v10) + eta * ((1.0 - xi) * v01 + xi * v11);
                        Jz[i] = f == 0 ? -pf : Jz[i] + pf;
                    }
                }
        }
        double acc[NP][D1Z];
#pragma unroll
        for (int n = 0; n < NP; ++n)
#pragma unroll
            for (int dz = 0; dz < D1Z; ++dz) acc[n][dz] = 0.0;
        const double idt = 1.0 / k.dt;
        const double wxy = sW[qx] * sW[qy];
        // 2c. the z points
#pragma unroll
        for (int qz = 0; qz < Q1Z; ++qz) {
            double bz[D1Z], gz[D1Z];
            if constexpr (DIM == 3) {
#pragma unroll
                for (int dz = 0; dz < D1Z; ++dz) {
                    bz[dz] = sB[qz][dz];
                    gz[dz] = sG[qz][dz];
                }
            } else {
                bz[0] = 1.0;
                gz[0] = 0.0;
            }
            double uq = 0.0, dq = 0.0, gu[DIM] = {}, vq = 0.0, gv[DIM] = {};
#pragma unroll
            for (int dz = 0; dz < D1Z; ++dz) {
                uq += bz[dz] * uv[dz];
                dq += bz[dz] * dv[dz];
                gu[0] += bz[dz] * ugx[dz];
                gu[1] += bz[dz] * ugy[dz];
                if constexpr (DIM == 3) gu[2] += gz[dz] * uw[dz];
                if constexpr (MODE == kNlJvp) {
                    vq += bz[dz] * vv[dz];
                    gv[0] += bz[dz] * vgx[dz];
                    gv[1] += bz[dz] * vgy[dz];
                    if constexpr (DIM == 3) gv[2] += gz[dz] * vv[dz];
                }
            }
            double J[DIM][DIM], A[DIM][DIM];
            double W = wxy;
            if constexpr (DIM == 3) {
                const double zeta = sPts[qz];
                W *= sW[qz];
#pragma unroll
                for (int i = 0; i < DIM; ++i) {
                    J[i][0] = (1.0 - zeta) * Jx[0][i] + zeta * Jx[1][i];
                    J[i][1] = (1.0 - zeta) * Jy[0][i] + zeta * Jy[1][i];
                    J[i][2] = Jz[i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < DIM; ++i) {
                    J[i][0] = Jx[0][i];
                    J[i][1] = Jy[0][i];
                }
            }
            const double det = adjugate<DIM>(J, A);
            const double au = k.a0 + k.a1 * (uq - k.u_ref), mu = k.m0 + k.m1 * (uq - k.u_ref);
            double tu[DIM];
            metric_flux<DIM>(A, W / det, gu, tu);
            if constexpr (MODE != kNlDiag) {
                double s, fl[DIM];
                if constexpr (MODE == kNlResidual) {
                    s = W * det * mu * dq * idt;
#pragma unroll
                    for (int b = 0; b < DIM; ++b) fl[b] = au * tu[b];
                } else {
                    double tv[DIM];
                    metric_flux<DIM>(A, W / det, gv, tv);
                    s = W * det * (mu + k.m1 * dq) * idt * vq;
#pragma unroll
                    for (int b = 0; b < DIM; ++b) fl[b] = au * tv[b] + (k.a1 * vq) * tu[b];
                }
#pragma unroll
                for (int dz = 0; dz < D1Z; ++dz) {
                    double p0 = bz[dz] * s;
                    if constexpr (DIM == 3) p0 += gz[dz] * fl[2];
                    acc[0][dz] += p0;
                    acc[1][dz] += bz[dz] * fl[0];
                    acc[2][dz] += bz[dz] * fl[1];
                }
            } else {
                const double Ms = W * det * (mu + k.m1 * dq) * idt, f = W * au / det;
                double D[DIM][DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a)
#pragma unroll
                    for (int b = 0; b < DIM; ++b) {
                        double s = 0.0;
#pragma unroll
                        for (int m = 0; m < DIM; ++m) s += A[a][m] * A[b][m];
                        D[a][b] = f * s;
                    }
#pragma unroll
                for (int dz = 0; dz < D1Z; ++dz) {
                    const double bb = bz[dz] * bz[dz];
                    double pa = Ms * bb, pe = (k.a1 * tu[0]) * bb, pf = (k.a1 * tu[1]) * bb;
                    if constexpr (DIM == 3) {
                        const double bg = bz[dz] * gz[dz];
                        pa += D[2][2] * (gz[dz] * gz[dz]) + (k.a1 * tu[2]) * bg;
                        pe += 2.0 * D[0][2] * bg;
                        pf += 2.0 * D[1][2] * bg;
                    }
                    acc[0][dz] += pa;                      // Bx^2 By^2
                    acc[1][dz] += D[0][0] * bb;            // Gx^2 By^2
                    acc[2][dz] += D[1][1] * bb;            // Bx^2 Gy^2
                    acc[3][dz] += 2.0 * D[0][1] * bb;      // BxGx ByGy
                    acc[4][dz] += pe;                      // BxGx By^2
                    acc[5][dz] += pf;                      // Bx^2 ByGy
                }
            }
        }
#pragma unroll
        for (int n = 0; n < NP; ++n)
#pragma unroll
            for (int dz = 0; dz < D1Z; ++dz) sP[el][n][dz][r] = acc[n][dz];
    }
    __syncthreads();
    // 3. the transposed x / y contraction, one local dof per thread and pass
    if (live) {
        const int slot = slot0 + el;
        double *yp = Ye + (size_t)(slot >> 6) * ND * kLanes + (slot & 63);
        for (int l = r; l < ND; l += TPE) {
            const int dx = l % D1, dy = (l / D1) % D1, dz = l / (D1 * D1);
            double y = 0.0;
            for (int qy = 0; qy < Q1; ++qy) {
                const double by = sB[qy][dy], gy = sG[qy][dy];
                double s0 = 0.0, s1 = 0.0;
                for (int qx = 0; qx < Q1; ++qx) {
                    const double bx = sB[qx][dx], gx = sG[qx][dx];
                    const int q = qx + Q1 * qy;
                    if constexpr (MODE != kNlDiag) {
                        s0 += bx * sP[el][0][dz][q] + gx * sP[el][1][dz][q];
                        s1 += bx * sP[el][2][dz][q];
                    } else {
                        const double bb = bx * bx, bg = bx * gx;
                        s0 += bb * sP[el][0][dz][q] + (gx * gx) * sP[el][1][dz][q] + bg * sP[el][4][dz][q];
                        s1 += bb * sP[el][5][dz][q] + bg * sP[el][3][dz][q];
                        y += (gy * gy) * (bb * sP[el][2][dz][q]);
                    }
                }
                if constexpr (MODE != kNlDiag) y += by * s0 + gy * s1;
                else y += (by * by) * s0 + (by * gy) * s1;
            }
            yp[(size_t)l * kLanes] = y;
        }
    }
}

// ---- launchers -----------------------------------------------------------------------------------
template <int DIM, int P>
static NlTab<P + 1, nl_tensor_points_1d(DIM, P)> nl_tab(const Rule1D &r)
{
    NlTab<P + 1, nl_tensor_points_1d(DIM, P)> t;
    for (int q = 0; q < r.q1; ++q) {
        for (int d = 0; d < r.d1; ++d) {
            t.B[q][d] = r.B[q][d];
            t.G[q][d] = r.G[q][d];
        }
        t.pts[q] = r.pts[q];
        t.w[q] = r.wts[q];
    }
    return t;
}

bool nl_tensor_supported(int dim, int p) { return dim == 2 ? (p >= 1 && p <= 3) : dim == 3 ? (p == 1 || p == 2) : false; }

// mode: 0 residual (Ye = the elements' shares of R at u), 1 jvp (of J(u) v), 2 diagonal (of J(u)'s diagonal)
hipError_t launch_nl_tensor(cdfem_ctx *c, int mode, const double *u, const double *v, bool con, double *Ye,
                            const KrylovState *st)
{
    const NlState &H = c->heat;
    const cdfem_nl_heat_coeffs k = nl_coeffs(c);
    const int nslots = c->nblk * kLanes;
    return dispatch_nl_tensor(c, [&](auto D, auto Pc) {
        constexpr int DIM = D(), P = Pc();
        const auto T = nl_tab<DIM, P>(H.rule);
        const dim3 grid((unsigned)((nslots + NlShape<DIM, P>::EPB - 1) / NlShape<DIM, P>::EPB)), block(256);
        return dispatch_value<0, 1, 2>(mode, hipErrorInvalidValue, [&](auto M) {
            // (a plain launch, as k_apply3d's: a profiling mark times both with the same event interval)
            hipLaunchKernelGGL((k_nl_tensor<DIM, P, M()>), grid, block, 0, c->stream, c->d_map.get(), c->d_perm.get(),
                               c->d_verts.get(), nslots, T, k, u, H.d_uold.get(), v, con ? 1 : 0, Ye, st);
            return hipGetLastError();
        });
    });
}

}  // namespace cdfem
