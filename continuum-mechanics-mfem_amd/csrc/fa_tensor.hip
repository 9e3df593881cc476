// fa_tensor.hip — full assembly on quad and hex meshes: the element matrices.
//
//   E(i, j) = a(phi_j, phi_i) = sum_q [ grad phi_i . D_q grad phi_j + phi_i (C_q . grad phi_j) + M_q phi_i phi_j ]
//
// with D = W adj(J) K adj(J)^T / det J, C = W alpha adj(J) c, M = W s det J in reference coordinates (the
// partial-assembly definitions of include/cdfem.h), on the one OPERATOR rule of the PA path (Gauss-Legendre,
// p + 1 points per direction on quads, p + 2 on hexes, q lexicographic with qx fastest), the GLL nodal basis
// and the multilinear map of the element's 2^dim vertices.  Everything after the element matrices is the
// simplex pipeline of fa_kernels.hip unchanged: the gather, the elimination, the SELL fill.
//
// Mapping: a wave is the 64 elements of one Ee block (lane = e % 64) times one row i (blockIdx.y).  The row
// index and the rule's tables are wave-uniform, the element's geometry and point data are per lane, and each
// lane keeps the row's nd entries in registers:
//   E(i, j) += (D grad phi_i + phi_i C) . grad phi_j + (M phi_i) phi_j        (D is symmetric)
// so a point costs the lane its geometry once and four multiply-adds per column.  The nd stores of a wave
// are 512 contiguous bytes each (the Ee layout puts e % 64 fastest): no LDS, no atomics, no scratch.  The
// geometry is formed again by each of the nd rows; the setup is not on the iteration path and the direct
// product is a few milliseconds on 262,144 Q2 hexes, so the simple kernel is kept over a sum-factorised one.
// Per-point coefficient arrays are read at (e * nq + q), a strided access the setup can afford.
#include <hip/hip_runtime.h>

#include "cdfem_internal.hpp"
#include "dispatch.hpp"

namespace cdfem {

bool fa_tensor_supported(int dim, int p) { return dim == 2 ? (p >= 1 && p <= 4) : (dim == 3 && (p == 1 || p == 2)); }

// J and x-independent pieces of the multilinear map at xi: J[i][k] = d x_i / d xi_k (lexicographic vertices:
// bit k of the vertex number is its position along axis k)
template <int DIM>
__device__ inline void tensor_jacobian(const double (&V)[(1 << DIM) * DIM], const double (&xi)[DIM], double (&J)[DIM][DIM])
{
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int k = 0; k < DIM; ++k) J[i][k] = 0.0;
#pragma unroll
    for (int v = 0; v < (1 << DIM); ++v) {
        double f[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) f[k] = ((v >> k) & 1) ? xi[k] : 1.0 - xi[k];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            double dN = ((v >> k) & 1) ? 1.0 : -1.0;
#pragma unroll
            for (int m = 0; m < DIM; ++m)
                if (m != k) dN *= f[m];
#pragma unroll
            for (int i = 0; i < DIM; ++i) J[i][k] += V[v * DIM + i] * dN;
        }
    }
}

template <int DIM>
__device__ inline double tensor_adjugate(const double (&J)[DIM][DIM], double (&A)[DIM][DIM])
{
    if constexpr (DIM == 2) {
        A[0][0] = J[1][1]; A[0][1] = -J[0][1];
        A[1][0] = -J[1][0]; A[1][1] = J[0][0];
        return J[0][0] * J[1][1] - J[0][1] * J[1][0];
    } else {
        A[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        A[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
        A[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
        A[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        A[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
        A[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
        A[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        A[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
        A[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        return J[0][0] * A[0][0] + J[0][1] * A[1][0] + J[0][2] * A[2][0];
    }
}

template <int DIM, int P>
__global__ void __launch_bounds__(64)
k_tensor_elem(const double *__restrict__ verts, int ne, const Rule1D r, unsigned kinds, double kappa,
              const double *__restrict__ kq, const double *__restrict__ kmq, double alpha, double c0, double c1,
              double c2, const double *__restrict__ cq, double mass, const double *__restrict__ mq,
              double *__restrict__ Ee)
{
    constexpr int D1 = P + 1, Q1 = DIM == 3 ? P + 2 : P + 1;
    constexpr int DZ = DIM == 3 ? D1 : 1, QZ = DIM == 3 ? Q1 : 1;
    constexpr int ND = D1 * D1 * DZ, NQ = Q1 * Q1 * QZ, NV = 1 << DIM;
    const int e = blockIdx.x * kLanes + threadIdx.x;
    const int i = blockIdx.y;  // the row: wave-uniform
    if (e >= ne) return;       // (padding lanes of the last block: their entries are never gathered)
    const int ix = i % D1, iy = (i / D1) % D1, iz = i / (D1 * D1);
    double V[NV * DIM];
#pragma unroll
    for (int k = 0; k < NV * DIM; ++k) V[k] = verts[(size_t)e * NV * DIM + k];
    double acc[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) acc[j] = 0.0;
    const double cc[3] = {c0, c1, c2};
    const bool dif = kinds & CDFEM_DIFFUSION, con = kinds & CDFEM_CONVECTION, mas = kinds & CDFEM_MASS;
#pragma unroll 1
    for (int q = 0; q < NQ; ++q) {
        const int qx = q % Q1, qy = (q / Q1) % Q1, qz = q / (Q1 * Q1);
        double xi[DIM], W = r.wts[qx] * r.wts[qy];
        xi[0] = r.pts[qx];
        xi[1] = r.pts[qy];
        if constexpr (DIM == 3) {
            xi[2] = r.pts[qz];
            W *= r.wts[qz];
        }
        double J[DIM][DIM], A[DIM][DIM];
        tensor_jacobian<DIM>(V, xi, J);
        const double det = tensor_adjugate<DIM>(J, A);
        const size_t eq = (size_t)e * NQ + q;
        // the row's basis function at the point: value and reference gradient
        const double bx = r.B[qx][ix], gx = r.G[qx][ix], by = r.B[qy][iy], gy = r.G[qy][iy];
        const double bz = DIM == 3 ? r.B[qz][iz] : 1.0, gz = DIM == 3 ? r.G[qz][iz] : 0.0;
        const double phi = bx * by * bz;
        double gi[DIM];
        gi[0] = gx * by * bz;
        gi[1] = bx * gy * bz;
        if constexpr (DIM == 3) gi[2] = bx * by * gz;
        // w = D grad phi_i + phi_i C, m = M phi_i
        double w[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) w[a] = 0.0;
        double m = 0.0;
        if (dif) {
            const double kap = kq ? kq[eq] : kappa;
            // t = adj(J)^T grad phi_i, then K t, then adj(J) (K t), scaled by W / det J
            double t[DIM], Kt[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                t[k] = 0.0;
#pragma unroll
                for (int a = 0; a < DIM; ++a) t[k] += A[a][k] * gi[a];
            }
#pragma unroll
            for (int k = 0; k < DIM; ++k) Kt[k] = kap * t[k];
            if (kmq) {  // MatrixCoefficient: K = kap I + K_q (symmetric, upper triangle by rows)
                constexpr int NS = DIM * (DIM + 1) / 2;
                double K[DIM][DIM];
#pragma unroll
                for (int k = 0, s = 0; k < DIM; ++k)
#pragma unroll
                    for (int l = k; l < DIM; ++l, ++s) K[k][l] = K[l][k] = kmq[eq * NS + s];
#pragma unroll
                for (int k = 0; k < DIM; ++k)
#pragma unroll
                    for (int l = 0; l < DIM; ++l) Kt[k] += K[k][l] * t[l];
            }
            const double s = W / det;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < DIM; ++k) v += A[a][k] * Kt[k];
                w[a] = s * v;
            }
        }
        if (con) {
            const double f = W * alpha * phi;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < DIM; ++k) v += A[a][k] * (cq ? cq[eq * DIM + k] : cc[k]);
                w[a] += f * v;
            }
        }
        if (mas) m = W * (mq ? mq[eq] : mass) * det * phi;
        // the row: acc[j] += w . grad phi_j + m phi_j, the y and z factors of column j shared along x
#pragma unroll
        for (int jz = 0; jz < DZ; ++jz)
#pragma unroll
            for (int jy = 0; jy < D1; ++jy) {
                const double Bz = DIM == 3 ? r.B[qz][jz] : 1.0, Gz = DIM == 3 ? r.G[qz][jz] : 0.0;
                const double byz = r.B[qy][jy] * Bz;
                const double t0 = w[0] * byz;  // times G_x
                double t1 = w[1] * (r.G[qy][jy] * Bz) + m * byz;  // times B_x
                if constexpr (DIM == 3) t1 += w[2] * (r.B[qy][jy] * Gz);
#pragma unroll
                for (int jx = 0; jx < D1; ++jx) acc[jx + D1 * (jy + D1 * jz)] += r.G[qx][jx] * t0 + r.B[qx][jx] * t1;
            }
    }
    // Ee[((e / 64) nd^2 + i nd + j) 64 + e % 64]: each j one 512-byte wave store
    double *out = Ee + ((size_t)blockIdx.x * ND * ND + (size_t)i * ND) * kLanes + threadIdx.x;
#pragma unroll
    for (int j = 0; j < ND; ++j) out[(size_t)j * kLanes] = acc[j];
}

hipError_t launch_tensor_elem(cdfem_ctx *c, const double *kq, const double *kmq, double kappa, double alpha,
                              const double *conv, const double *cq, const double *mq, double mass)
{
    if (!fa_tensor_supported(c->dim, c->p)) return hipErrorInvalidValue;
    if (c->rule_op.q1 != (c->dim == 3 ? c->p + 2 : c->p + 1)) return hipErrorInvalidValue;
    const dim3 g((c->ne + kLanes - 1) / kLanes, c->nd), b(kLanes);
    const double c0 = conv ? conv[0] : 0.0, c1 = conv ? conv[1] : 0.0, c2 = (conv && c->dim == 3) ? conv[2] : 0.0;
    return dispatch_value<21, 22, 23, 24, 31, 32>(10 * c->dim + c->p, hipErrorInvalidValue, [&](auto DP) {
        hipLaunchKernelGGL((k_tensor_elem<DP() / 10, DP() % 10>), g, b, 0, c->stream, c->d_verts.get(), c->ne,
                           c->rule_op, c->kinds, kappa, kq, kmq, alpha, c0, c1, c2, cq, mass, mq, c->d_Ee.get());
        return hipGetLastError();
    });
}

}  // namespace cdfem
