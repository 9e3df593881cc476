// point_geom.hpp — the pointwise geometry of the setup and assembly kernels, written once (pa_kernels.hip,
// fa_kernels.hip, fa_tensor.hip, nl_kernels.hip, nl_tensor.hip, nl_fa_tensor.hip): adj(J) and det J, the affine
// simplex map, the multilinear map of a quad's or hex's 2^dim vertices, f adj(J) adj(J)^T applied to a reference
// gradient, a tensor space's sizes, the decode of a tensor rule's point, and the row kernel both full assemblies on
// quads and hexes run.  (The tuned applies form their factors from cross products of the map's columns: pa_core.hpp,
// ho_kernels.hip.)
#pragma once
#include "cdfem_internal.hpp"

namespace cdfem {

// adj(J) (A[a][k] = det J d xi_a / d x_k) and det J; J[k][m] = d x_k / d xi_m
template <int DIM>
__device__ __forceinline__ double adjugate(const double (&J)[DIM][DIM], double (&A)[DIM][DIM])
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

// the same of the affine map of a simplex's vertices V: J[k][m] = V[(m + 1) DIM + k] - V[k]
template <int DIM>
__device__ __forceinline__ double simplex_adjugate(const double *__restrict__ V, double (&A)[DIM][DIM])
{
    double J[DIM][DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k)
#pragma unroll
        for (int m = 0; m < DIM; ++m) J[k][m] = V[(m + 1) * DIM + k] - V[k];
    return adjugate<DIM>(J, A);
}

// the multilinear map of the 2^DIM vertices V at xi (lexicographic vertices: bit k of the vertex number is its
// position along axis k): J[i][k] = d x_i / d xi_k and, where x is given, the point itself
template <int DIM>
__device__ __forceinline__ void multilinear_map(const double *__restrict__ V, const double (&xi)[DIM],
                                                double (&J)[DIM][DIM], double *x = nullptr)
{
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
        if (x) x[i] = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) J[i][k] = 0.0;
    }
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
        if (x) {
            double N = 1.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) N *= f[k];
#pragma unroll
            for (int i = 0; i < DIM; ++i) x[i] += V[v * DIM + i] * N;
        }
    }
}

// t[b] = f sum_k A[b][k] (sum_a A[a][k] g[a]): f adj(J) adj(J)^T applied to a reference gradient
template <int DIM>
__device__ __forceinline__ void metric_flux(const double (&A)[DIM][DIM], double f, const double (&g)[DIM], double (&t)[DIM])
{
    double gk[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        gk[k] = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) gk[k] += A[a][k] * g[a];
    }
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) s += A[b][k] * gk[k];
        t[b] = f * s;
    }
}

// the sizes of the degree-P space on a quad or hex under a rule of Q1 points per direction
template <int DIM, int P, int Q1_>
struct TensorShape {
    static constexpr int D1 = P + 1;
    static constexpr int Q1 = Q1_;
    static constexpr int DZ = DIM == 3 ? D1 : 1;
    static constexpr int QZ = DIM == 3 ? Q1 : 1;
    static constexpr int ND = D1 * D1 * DZ;
    static constexpr int NQ = Q1 * Q1 * QZ;
    static constexpr int NV = 1 << DIM;
};

// point q of the tensor rule r with q1 points per direction (q lexicographic, qx fastest): its 1D indices, its
// reference coordinates and its weight
template <int DIM>
__device__ __forceinline__ void tensor_point(int q, int q1, const Rule1D &r, int (&qi)[3], double (&xi)[DIM], double &W)
{
    qi[0] = q % q1;
    qi[1] = (q / q1) % q1;
    qi[2] = q / (q1 * q1);
    xi[0] = r.pts[qi[0]];
    xi[1] = r.pts[qi[1]];
    W = r.wts[qi[0]] * r.wts[qi[1]];
    if constexpr (DIM == 3) {
        xi[2] = r.pts[qi[2]];
        W *= r.wts[qi[2]];
    }
}

// Row i = blockIdx.y of the element matrices of a form on quads or hexes,
//   E(i, j) = sum_q [ w_q . grad_ref phi_j + m_q phi_j ],
// for the 64 elements of one Ee block (lane = e % 64; launch: 64 threads, grid (blocks of 64 elements, nd rows)).
// The row index and the rule's tables are wave-uniform, the element's geometry (the multilinear map of its 2^dim
// vertices, formed at every point) is per lane, and each lane keeps the row's nd entries in registers: a point costs
// the lane its geometry once and four multiply-adds per column.  The nd stores of a wave are 512 contiguous bytes
// each (the Ee layout puts e % 64 fastest): no LDS, no atomics, no scratch, one fixed summation order.
// point(e, q, W, det, A, phi, gi, w, m) fills w[DIM] and m for the row's function (value phi, reference gradient gi)
// at point q of element e, from the point's weight W, det J and A = adj(J).
template <int DIM, int P, int Q1, class PointFn>
__device__ __forceinline__ void tensor_elem_row(const double *__restrict__ verts, int ne, const Rule1D &r,
                                                PointFn &&point, double *__restrict__ Ee)
{
    using S = TensorShape<DIM, P, Q1>;
    constexpr int D1 = S::D1, DZ = S::DZ, ND = S::ND, NQ = S::NQ, NV = S::NV;
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
#pragma unroll 1
    for (int q = 0; q < NQ; ++q) {
        int qi[3];
        double xi[DIM], W;
        tensor_point<DIM>(q, Q1, r, qi, xi, W);
        const int qx = qi[0], qy = qi[1], qz = qi[2];
        double J[DIM][DIM], A[DIM][DIM];
        multilinear_map<DIM>(V, xi, J);
        const double det = adjugate<DIM>(J, A);
        // the row's basis function at the point: value and reference gradient
        const double bx = r.B[qx][ix], gx = r.G[qx][ix], by = r.B[qy][iy], gy = r.G[qy][iy];
        const double bz = DIM == 3 ? r.B[qz][iz] : 1.0, gz = DIM == 3 ? r.G[qz][iz] : 0.0;
        const double phi = bx * by * bz;
        double gi[DIM];
        gi[0] = gx * by * bz;
        gi[1] = bx * gy * bz;
        if constexpr (DIM == 3) gi[2] = bx * by * gz;
        double w[DIM], m;
        point(e, q, W, det, A, phi, gi, w, m);
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

}  // namespace cdfem
