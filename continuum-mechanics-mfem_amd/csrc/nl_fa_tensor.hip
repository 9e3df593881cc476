// nl_fa_tensor.hip — the nonlinear heat form's Jacobian on quads and hexes as element matrices (cdfem_nl_fa_setup,
// DESIGN.md §4.8a), and the boundary linear form on their faces.
//
//   a(u) = a0 + a1 (u - u_ref),  m(u) = m0 + m1 (u - u_ref),  mu = (m(u) + m1 (u - u_old)) / dt.
//   In reference coordinates, with A = adj(J), s = W / det J and g_i the reference gradient of phi_i:
//   J_ij = sum_q [ a(u) s (A A^T g_i) . g_j + ( W det mu phi_i + a1 s (A A^T g_i) . g_u ) phi_j ]
//
// on the rule of nl_tensor.hip (Gauss-Legendre, p + 2 points per direction on quads, p + 3 on hexes, q
// lexicographic with qx fastest), the GLL nodal basis and the multilinear map of the element's 2^dim vertices.
// The a1 term is the transpose of a convection term (the velocity multiplies the row's gradient, not the
// column's), which no per-point coefficient array of k_tensor_elem expresses; everything else is that kernel.
//
// Two kernels per Jacobian:
//   k_nl_tensor_point  one thread per (element, point): a(u), mu and the reference gradient of u at the point,
//                      2 + dim doubles into d_jq[e / 64][q][2 + dim][e % 64].  u - u_old is interpolated from the
//                      per-dof differences and the gradient is taken of u - u(dof 0), as k_nl_tensor does
//                      (nl_kernels.hip nl_point says why).
//   k_nl_tensor_elem   the row core of point_geom.hpp (tensor_elem_row, as k_tensor_elem) with this form's point
//                      functor: with t = s A A^T g_i,
//                        w = a(u) t,   m = W det mu phi_i + a1 (t . g_u),
//                      the point state read in 512-byte wave loads.
// The point state is formed once and read by all nd rows: forming it in the row kernel would cost every row the
// nd-term interpolations again and hold the element's 2 nd dof values next to the nd accumulators.
// No LDS, no atomics, no scratch, one fixed summation order.
//
// k_bdr_lf_tensor: BoundaryLFIntegrator on facet t = (element, f = 2 axis + side), one thread per facet: the
// facet's (p + 1)^(dim - 1) dofs are the element's lexicographic dofs with axis index 0 or p (lower remaining axis
// fastest), the rule is tensor Gauss-Legendre with n = (p + 1) / 2 + 1 points per direction, and the measure
// factor is formed at every point from the element's vertices: |dx/ds| on an edge, |dx/ds x dx/dt| on a
// (bilinear) face.  The facet E-vector is summed by k_bdr_gather, as on simplices.
#include <hip/hip_runtime.h>

#include "cdfem_internal.hpp"
#include "point_geom.hpp"

namespace cdfem {

namespace {

template <int DIM, int P>
struct NlFaShape : TensorShape<DIM, P, nl_tensor_points_1d(DIM, P)> {
    static constexpr int NC = 2 + DIM;  // a(u), mu, the reference gradient of u
};

}  // namespace

// the point state of J(u): grid (blocks of 64 elements, points), the point wave-uniform
template <int DIM, int P>
__global__ void __launch_bounds__(64)
k_nl_tensor_point(const int32_t *__restrict__ edofs, int ne, const Rule1D r, cdfem_nl_heat_coeffs k,
                  const double *__restrict__ u, const double *__restrict__ uold, double *__restrict__ jq)
{
    using S = NlFaShape<DIM, P>;
    constexpr int D1 = S::D1, Q1 = S::Q1, DZ = S::DZ, ND = S::ND, NQ = S::NQ, NC = S::NC;
    const int e = blockIdx.x * kLanes + threadIdx.x;
    const int q = blockIdx.y;
    if (e >= ne) return;  // (padding lanes of the last block: the row kernel leaves them too)
    const int qx = q % Q1, qy = (q / Q1) % Q1, qz = q / (Q1 * Q1);
    const int32_t *ed = edofs + (size_t)e * ND;
    const double u0 = u[ed[0]];
    double uq = 0.0, dq = 0.0, gu[DIM] = {};
#pragma unroll
    for (int lz = 0; lz < DZ; ++lz)
#pragma unroll
        for (int ly = 0; ly < D1; ++ly) {
            const double Bz = DIM == 3 ? r.B[qz][lz] : 1.0, Gz = DIM == 3 ? r.G[qz][lz] : 0.0;
            const double byz = r.B[qy][ly] * Bz, gyz = r.G[qy][ly] * Bz;
            [[maybe_unused]] const double bgz = r.B[qy][ly] * Gz;
#pragma unroll
            for (int lx = 0; lx < D1; ++lx) {
                const int32_t g = ed[lx + D1 * (ly + D1 * lz)];
                const double ul = u[g], dl = ul - uold[g], wl = ul - u0;
                const double bx = r.B[qx][lx], gx = r.G[qx][lx];
                uq += (bx * byz) * ul;
                dq += (bx * byz) * dl;
                gu[0] += (gx * byz) * wl;
                gu[1] += (bx * gyz) * wl;
                if constexpr (DIM == 3) gu[2] += (bx * bgz) * wl;
            }
        }
    const double au = k.a0 + k.a1 * (uq - k.u_ref), mu = (k.m0 + k.m1 * (uq - k.u_ref) + k.m1 * dq) / k.dt;
    double *out = jq + ((size_t)blockIdx.x * NQ + q) * NC * kLanes + threadIdx.x;
    out[0] = au;
    out[kLanes] = mu;
#pragma unroll
    for (int a = 0; a < DIM; ++a) out[(size_t)(2 + a) * kLanes] = gu[a];
}

// row i of the element matrices of J(u): grid (blocks of 64 elements, nd rows)
template <int DIM, int P>
__global__ void __launch_bounds__(64)
k_nl_tensor_elem(const double *__restrict__ verts, int ne, const Rule1D r, double a1, const double *__restrict__ jq,
                 double *__restrict__ Ee)
{
    using S = NlFaShape<DIM, P>;
    constexpr int NQ = S::NQ, NC = S::NC;
    const double *pq = jq + (size_t)blockIdx.x * NQ * NC * kLanes + threadIdx.x;
    tensor_elem_row<DIM, P, S::Q1>(verts, ne, r, [&](int, int q, double W, double det, const double (&A)[DIM][DIM],
                                                     double phi, const double (&gi)[DIM], double (&w)[DIM], double &m) {
        // the point state
        const double *sq = pq + (size_t)q * NC * kLanes;
        const double au = sq[0], mu = sq[kLanes];
        double gu[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) gu[a] = sq[(size_t)(2 + a) * kLanes];
        // t = s A A^T g_i
        double t[DIM], tg = 0.0;
        metric_flux<DIM>(A, W / det, gi, t);
#pragma unroll
        for (int b = 0; b < DIM; ++b) tg += t[b] * gu[b];
#pragma unroll
        for (int b = 0; b < DIM; ++b) w[b] = au * t[b];
        m = (W * det) * mu * phi + a1 * tg;
    }, Ee);
}

size_t nl_fa_tensor_state_size(const cdfem_ctx *c)
{
    return (size_t)((c->ne + kLanes - 1) / kLanes) * nq_of(c, c->heat.rule) * (2 + c->dim) * kLanes;
}

// d_Ee = the element matrices of J(u); u_old, the rule and the coefficients from c->heat
hipError_t launch_nl_tensor_elem(cdfem_ctx *c, const double *u)
{
    const NlState &H = c->heat;
    if (H.rule.q1 != nl_tensor_points_1d(c->dim, c->p) || !H.d_jq || !H.d_edofs || !c->d_Ee) return hipErrorInvalidValue;
    const unsigned nb = (unsigned)((c->ne + kLanes - 1) / kLanes);
    return dispatch_nl_tensor(c, [&](auto D, auto Pc) {
        constexpr int DIM = D(), P = Pc();
        hipLaunchKernelGGL((k_nl_tensor_point<DIM, P>), dim3(nb, NlFaShape<DIM, P>::NQ), dim3(kLanes), 0, c->stream,
                           H.d_edofs.get(), c->ne, H.rule, nl_coeffs(c), u, H.d_uold.get(), H.d_jq.get());
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_nl_tensor_elem<DIM, P>), dim3(nb, NlFaShape<DIM, P>::ND), dim3(kLanes), 0, c->stream,
                           c->d_verts.get(), c->ne, H.rule, H.a1, H.d_jq.get(), c->d_Ee.get());
        return hipGetLastError();
    });
}

// ---- the boundary linear form on quad / hex faces ------------------------------------------------------
// btab: B[n][p + 1] (the 1D basis at the facet rule's points), then pts[n], then w[n]
template <int DIM, int P>
__global__ void __launch_bounds__(64)
k_bdr_lf_tensor(const double *__restrict__ verts, const int32_t *__restrict__ face_elem,
                const int32_t *__restrict__ face_local, int nbf, int n1, const double *__restrict__ btab,
                const double *__restrict__ gq, double *__restrict__ Ye)
{
    constexpr int D1 = P + 1, NV = 1 << DIM, NF = DIM == 3 ? D1 * D1 : D1;
    const int t = blockIdx.x * kLanes + threadIdx.x;
    if (t >= nbf) return;
    const int f = face_local[t], axis = f >> 1, side = f & 1;
    const double *V = verts + (size_t)face_elem[t] * NV * DIM;
    // the facet's 2^(dim - 1) vertices, lower remaining axis fastest
    const int a0 = axis == 0 ? 1 : 0, a1 = DIM == 3 ? (axis == 2 ? 1 : 2) : 0;
    double X[NV / 2][DIM];
#pragma unroll
    for (int m = 0; m < NV / 2; ++m) {
        int v = side << axis;
        v |= (m & 1) << a0;
        if constexpr (DIM == 3) v |= ((m >> 1) & 1) << a1;
#pragma unroll
        for (int k = 0; k < DIM; ++k) X[m][k] = V[v * DIM + k];
    }
    const double *Bt = btab, *pts = btab + (size_t)n1 * D1, *wts = pts + n1;
    double b[NF];
#pragma unroll
    for (int l = 0; l < NF; ++l) b[l] = 0.0;
    const int nqb = DIM == 3 ? n1 * n1 : n1;
    for (int q = 0; q < nqb; ++q) {
        const int qs = q % n1, qt = q / n1;
        double meas, W = wts[qs];
        if constexpr (DIM == 2) {
            const double dx = X[1][0] - X[0][0], dy = X[1][1] - X[0][1];
            meas = sqrt(dx * dx + dy * dy);
        } else {
            const double sx = pts[qs], tx = pts[qt];
            W *= wts[qt];
            double ts[3], tt[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ts[k] = (1.0 - tx) * (X[1][k] - X[0][k]) + tx * (X[3][k] - X[2][k]);
                tt[k] = (1.0 - sx) * (X[2][k] - X[0][k]) + sx * (X[3][k] - X[1][k]);
            }
            const double cx = ts[1] * tt[2] - ts[2] * tt[1], cy = ts[2] * tt[0] - ts[0] * tt[2],
                         cz = ts[0] * tt[1] - ts[1] * tt[0];
            meas = sqrt(cx * cx + cy * cy + cz * cz);
        }
        const double fw = W * meas * gq[(size_t)t * nqb + q];
#pragma unroll
        for (int lt = 0; lt < (DIM == 3 ? D1 : 1); ++lt) {
            const double ft = DIM == 3 ? fw * Bt[qt * D1 + lt] : fw;
#pragma unroll
            for (int ls = 0; ls < D1; ++ls) b[ls + D1 * lt] += ft * Bt[qs * D1 + ls];
        }
    }
#pragma unroll
    for (int l = 0; l < NF; ++l) Ye[(size_t)t * NF + l] = b[l];
}

// the facet E-vector of a quad / hex mesh (launch_bdr_lf gathers it)
hipError_t launch_bdr_lf_tensor(cdfem_ctx *c, const double *gq)
{
    const NlState &H = c->heat;
    return dispatch_nl_tensor(c, [&](auto D, auto P) {
        hipLaunchKernelGGL((k_bdr_lf_tensor<D(), P()>), dim3((unsigned)((H.nbf + kLanes - 1) / kLanes)),
                           dim3(kLanes), 0, c->stream, c->d_verts.get(), H.d_face_elem.get(), H.d_face_local.get(),
                           H.nbf, H.nqb1, H.d_btab.get(), gq, H.d_bYe.get());
        return hipGetLastError();
    });
}

}  // namespace cdfem
