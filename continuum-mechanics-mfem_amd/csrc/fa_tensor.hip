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
// The kernel is the row core of point_geom.hpp (tensor_elem_row: the wave and row mapping, the geometry, the column
// loop and the Ee stores) with this form's point functor:
//   E(i, j) += (D grad phi_i + phi_i C) . grad phi_j + (M phi_i) phi_j        (D is symmetric)
// The geometry is formed again by each of the nd rows; the setup is not on the iteration path and the direct
// product is a few milliseconds on 262,144 Q2 hexes, so the simple kernel is kept over a sum-factorised one.
// Per-point coefficient arrays are read at (e * nq + q), a strided access the setup can afford.
#include <hip/hip_runtime.h>

#include "cdfem_internal.hpp"
#include "dispatch.hpp"
#include "point_geom.hpp"

namespace cdfem {

bool fa_tensor_supported(int dim, int p) { return dim == 2 ? (p >= 1 && p <= 4) : (dim == 3 && (p == 1 || p == 2)); }

template <int DIM, int P>
__global__ void __launch_bounds__(64)
k_tensor_elem(const double *__restrict__ verts, int ne, const Rule1D r, unsigned kinds, double kappa,
              const double *__restrict__ kq, const double *__restrict__ kmq, double alpha, double c0, double c1,
              double c2, const double *__restrict__ cq, double mass, const double *__restrict__ mq,
              double *__restrict__ Ee)
{
    constexpr int Q1 = DIM == 3 ? P + 2 : P + 1, NQ = TensorShape<DIM, P, Q1>::NQ;
    const double cc[3] = {c0, c1, c2};
    const bool dif = kinds & CDFEM_DIFFUSION, con = kinds & CDFEM_CONVECTION, mas = kinds & CDFEM_MASS;
    tensor_elem_row<DIM, P, Q1>(verts, ne, r, [&](int e, int q, double W, double det, const double (&A)[DIM][DIM],
                                                  double phi, const double (&gi)[DIM], double (&w)[DIM], double &m) {
        const size_t eq = (size_t)e * NQ + q;
        // w = D grad phi_i + phi_i C, m = M phi_i
#pragma unroll
        for (int a = 0; a < DIM; ++a) w[a] = 0.0;
        m = 0.0;
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
    }, Ee);
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
